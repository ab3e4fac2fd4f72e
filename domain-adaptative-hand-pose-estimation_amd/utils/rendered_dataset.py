"""A rendered two-domain hand data set that needs nothing on disk: every item is one fixed-size record (``mi355.ops.HAND_REC_DTYPE``,
include/mi355pose.h ``mi355_hand_rec``) from which ``mi355.ops.render_hands`` draws the image on the GPU, and the key points are
exact because they are the joints of the model that is drawn (utils/hand_model.py).  Host code, numpy float64; no pixels here.

``domain='cg'`` is the source: a flat two-colour background, no occluder, no sensor noise, a narrow skin / light range, gain 1 and
bias 0.  ``domain='photo'`` is the target: a value-noise background, wider skin and light ranges, an occluder with some
probability, sensor noise and per-channel gain / bias jitter.  ``gap`` in [0, 1] moves every 'photo' distribution from the 'cg'
one (0) to the full one (1); it does nothing to 'cg'.

Item i is a pure function of (seed, i, domain, gap): nothing needs checkpointing and a resumed run sees the same items.
Everything that needs sin, cos, exp or log is computed here and carried in the record.

Sequence mode (``hand_sequence`` / ``render_sequence``, predict.py --synthetic-hands-video): two drawn hands interpolated linearly in
joint positions, depths and radii over N frames of one 'photo' scene, rendered and converted to uint8 HWC frames on the device, so
that the key points of every frame of a video are exact as well."""
import numpy as np
from torch.utils.data import Dataset

from mi355.ops import HAND_REC_DTYPE
from . import hand_model as hm
from .synthetic_dataset import HAND_GROUPS

DOMAINS = ('cg', 'photo')

# ---- style ranges: (cg lo, cg hi), (photo lo, photo hi); a 'photo' draw at gap g is uniform in cg + g * (photo - cg) -------------
SKIN_LIGHT = (0.96, 0.80, 0.69)                     # the two ends of the skin-tone line the tone draw interpolates
SKIN_DARK = (0.45, 0.30, 0.22)
SKIN_TONE = ((0.40, 0.60), (0.0, 1.0))              # cg renders use a few mid tones, photographs the whole line
SKIN_JITTER = ((0.0, 0.0), (-0.05, 0.05))           # per-channel offset: cameras disagree about white balance
LIGHT_ANGLE = ((0.0, 15.0), (0.0, 60.0))            # degrees between the light and the camera axis: cg is lit from the camera
AMBIENT = ((0.45, 0.55), (0.20, 0.60))              # ambient share of the shading: photographs include hard light
BG_DARK = ((0.15, 0.35), (0.0, 1.0))                # channel range of the background's first colour: cg a dark grey, photo any
BG_BRIGHT = ((0.50, 0.70), (0.0, 1.0))              # ... and of its second colour
NOISE_AMP = ((0.0, 0.0), (0.10, 0.50))              # value-noise amplitude: cg backgrounds are flat, photo ones cluttered
NOISE_CELL_SHARE = (1.0 / 16, 1.0 / 4)              # lattice cell as a share of the side: clutter at the scale of a finger to a palm
OCCLUDER_PROB = (0.0, 0.35)                         # a held object hides part of the hand in about a third of the photographs
OCCLUDER_RADIUS_SHARE = (0.04, 0.09)                # its radius as a share of the side: a pen to a cup
SENSOR_SIGMA = ((0.0, 0.0), (0.01, 0.05))           # sensor noise, in units of the [0, 1] pixel range (its std is sigma / sqrt(3))
GAIN = ((1.0, 1.0), (0.75, 1.25))                   # per-channel photometric gain: exposure and white balance
BIAS = ((0.0, 0.0), (-0.08, 0.08))                  # per-channel black-level offset


def _range(r, g):
    (a0, a1), (b0, b1) = r
    return a0 + g * (b0 - a0), a1 + g * (b1 - a1)


class RenderedHand21(Dataset):
    num_keypoints = 21
    keypoints_group = HAND_GROUPS
    records_on_device = True            # items are records: utils.data.record_collate packs them, RenderedHandIterator draws them

    def __init__(self, length=4096, image_size=(256, 256), heatmap_size=(64, 64), sigma=2, seed=1, domain='cg', gap=1.0, **_):
        if domain not in DOMAINS:
            raise ValueError('RenderedHand21: domain must be one of %s, got %r' % (DOMAINS, domain))
        if not 0.0 <= float(gap) <= 1.0:
            raise ValueError('RenderedHand21: gap must be in [0, 1], got %r' % (gap,))
        if isinstance(image_size, int):
            image_size = (image_size, image_size)
        if isinstance(heatmap_size, int):
            heatmap_size = (heatmap_size, heatmap_size)
        if image_size[0] != image_size[1]:
            raise ValueError('RenderedHand21: the renderer draws square images, got %r' % (image_size,))
        self.length, self.image_size, self.heatmap_size, self.sigma, self.seed = int(length), tuple(image_size), tuple(heatmap_size), sigma, int(seed)
        self.domain, self.gap = domain, float(gap)

    def __len__(self):
        return self.length

    def _key(self, i):
        gap = self.gap if self.domain == 'photo' else 0.0        # gap does nothing to 'cg': its items are the same at every gap
        return [self.seed, int(i), DOMAINS.index(self.domain), int(round(gap * (1 << 20)))]

    def pose(self, i):
        """The pose draws of item i (utils.hand_model.draw_pose): the first draws of the item's generator."""
        return hm.draw_pose(np.random.default_rng(self._key(i)))

    def __getitem__(self, i):
        if not 0 <= i < self.length:
            raise IndexError(i)
        rng = np.random.default_rng(self._key(i))
        S = self.image_size[0]
        g = self.gap if self.domain == 'photo' else 0.0
        P, radius, _ = hm.project(hm.draw_pose(rng), S)

        def u(r, size=None):
            lo, hi = _range(r, g)
            return rng.uniform(lo, hi, size)

        rec = np.zeros((), dtype=HAND_REC_DTYPE)
        rec['jx'], rec['jy'], rec['jz'], rec['radius'] = P[:, 0], P[:, 1], P[:, 2], radius
        tone = u(SKIN_TONE)
        rec['skin'] = np.clip(np.array(SKIN_DARK) + tone * (np.array(SKIN_LIGHT) - np.array(SKIN_DARK)) + u(SKIN_JITTER, 3), 0.0, 1.0)
        alpha, beta = np.deg2rad(u(LIGHT_ANGLE)), rng.uniform(0.0, 2.0 * np.pi)
        rec['light'] = (np.sin(alpha) * np.cos(beta), np.sin(alpha) * np.sin(beta), np.cos(alpha))
        rec['ambient'] = u(AMBIENT)
        rec['bg0'], rec['bg1'] = u(BG_DARK, 3), u(BG_BRIGHT, 3)
        ga = rng.uniform(0.0, 2.0 * np.pi)
        grad = np.array([np.cos(ga), np.sin(ga)]) / S                 # the blend runs 0 .. 1 across about one image side
        rec['grad'], rec['grad_off'] = grad, 0.5 - float(grad.sum()) * (S - 1) / 2.0
        rec['noise_amp'] = u(NOISE_AMP)
        rec['noise_inv_cell'] = 1.0 / max(1.0, S * rng.uniform(*NOISE_CELL_SHARE))
        rec['noise_seed'] = rng.integers(0, 1 << 32, dtype=np.uint64)
        # the occluder: a capsule through the neighbourhood of the hand's centre, in front of its nearest joint or among them
        have = rng.uniform() < OCCLUDER_PROB[0] + g * (OCCLUDER_PROB[1] - OCCLUDER_PROB[0])
        c, oa, ol = P[:, :2].mean(axis=0) + rng.uniform(-0.15, 0.15, 2) * S, rng.uniform(0.0, 2.0 * np.pi), rng.uniform(0.2, 0.6) * S
        orad, oz = S * rng.uniform(*OCCLUDER_RADIUS_SHARE), rng.uniform(P[:, 2].min() - 0.1 * S, P[:, 2].mean())
        ocol = rng.uniform(0.0, 1.0, 3)
        if have:
            d = 0.5 * ol * np.array([np.cos(oa), np.sin(oa)])
            rec['occ_a'], rec['occ_b'], rec['occ_r'], rec['occ_z'], rec['occ_col'] = c - d, c + d, orad, oz, ocol
        rec['sensor_sigma'] = u(SENSOR_SIGMA)
        rec['sensor_seed'] = rng.integers(0, 1 << 32, dtype=np.uint64)
        rec['gain'], rec['bias'] = u(GAIN, 3), u(BIAS, 3)
        kp = np.stack([rec['jx'], rec['jy']], axis=1).astype(np.float32)
        visible = ((kp >= -0.5) & (kp < S - 0.5)).all(axis=1).astype(np.float32)[:, None]
        return rec, kp, visible

    def group_accuracy(self, accuracies):
        return {name: sum(accuracies[i] for i in ks) / len(ks) for name, ks in self.keypoints_group.items()}


def hand_sequence(n_frames, frame_size=256, seed=1, hand_share=0.45, travel=0.18, gap=1.0):
    """(records (n_frames,) of HAND_REC_DTYPE, key points (n_frames, 21, 2) fp32 in frame pixels) of a hand that moves and changes
    pose across a frame_size x frame_size frame.  Items 0 and 1 of RenderedHand21(domain='photo', seed) give the two poses: each
    is shrunk to `hand_share` of the frame about its centre and moved `travel` of the side away from it, one up and to the left,
    the other down and to the right; frame t interpolates joint positions, depths and radii linearly between them.  The scene
    (skin, light, background, gain and bias) is item 0's in every frame, without an occluder; the sensor noise is drawn anew per frame."""
    n_frames, S = int(n_frames), int(frame_size)
    if n_frames < 1:
        raise ValueError('hand_sequence: n_frames must be at least 1, got %r' % (n_frames,))
    ds = RenderedHand21(length=2, image_size=S, domain='photo', seed=seed, gap=gap)
    ends = []
    for i, sign in ((0, -1.0), (1, 1.0)):
        rec = ds[i][0]
        c = (S - 1) / 2.0
        shift = sign * travel * S * np.array([1.0, 0.6])
        ends.append((c + hand_share * (rec['jx'].astype(np.float64) - c) + shift[0], c + hand_share * (rec['jy'].astype(np.float64) - c) + shift[1],
                     hand_share * rec['jz'].astype(np.float64), hand_share * rec['radius'].astype(np.float64)))
    recs = np.zeros(n_frames, dtype=HAND_REC_DTYPE)
    recs[:] = ds[0][0]
    for t in range(n_frames):
        a = t / (n_frames - 1) if n_frames > 1 else 0.0
        for name, v0, v1 in zip(('jx', 'jy', 'jz', 'radius'), ends[0], ends[1]):
            recs[name][t] = (1.0 - a) * v0 + a * v1
    recs['occ_r'] = 0.0
    recs['sensor_seed'] = (int(recs['sensor_seed'][0]) + np.arange(n_frames, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return recs, np.stack([recs['jx'], recs['jy']], axis=2).astype(np.float32)


def render_sequence(recs, frame_size, device, chunk=16):
    """The uint8 (n, frame_size, frame_size, 3) RGB frames of `recs` on `device`: mi355_render_hands, de-normalised, rounded and
    laid out HWC by device operations (the host sees no pixel)."""
    import torch
    from mi355 import ops
    from mi355.augment import MEAN, STD
    S = int(frame_size)
    mean, std = (torch.tensor(v, dtype=torch.float32, device=device).view(1, 3, 1, 1) for v in (MEAN, STD))
    out = torch.empty((len(recs), S, S, 3), dtype=torch.uint8, device=device)
    for at in range(0, len(recs), chunk):
        part = np.ascontiguousarray(recs[at:at + chunk])
        r_d = torch.from_numpy(part.view(np.uint8).reshape(len(part), -1).copy()).to(device)
        x = ops.render_hands(r_d, S)
        out[at:at + len(part)] = ((x * std + mean).clamp_(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).permute(0, 2, 3, 1)
    return out
