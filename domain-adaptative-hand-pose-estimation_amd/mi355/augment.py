"""The training augmentation chain on the GPU (csrc/augment.hip, include/mi355pose.h ``mi355_augment``).

The host draws the parameters of every sample (``uda.dataset.keypoint_detection.DeviceAugment``, the same RNG calls as
the CPU chain) and ships the un-augmented uint8 RGB sources packed into one flat buffer; ``augment`` turns a batch of them
into the network input -- and optionally ``image_ema`` -- bit-identical with the Pillow chain
RandomRotation -> RandomResizedCrop -> ColorJitter -> GaussianBlur -> ToTensor -> Normalize.

One parameter row per image (float64, ``PARAM_COLUMNS``): rotation angle in degrees, crop top / left / side in the
rotated image, brightness / contrast / saturation factors, the op order (0 brightness, 1 contrast, 2 saturation; -1 for
no op) and the Gaussian blur radius.  The host turns each row into the record the kernels read, with the parts Pillow
computes on its host side done the way Pillow does them (the rotation matrix and its 16.16 fixed point, the box-blur
weights)."""
import math

import numpy as np
import torch

from . import call, load, ptr, stream_ptr, Mi355Error

PARAM_COLUMNS = ('angle', 'top', 'left', 'side', 'brightness', 'contrast', 'saturation', 'op0', 'op1', 'op2', 'blur')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# include/mi355pose.h mi355_aug_rec
REC = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4'), ('rot', '<i4'), ('a', '<i4', 6), ('top', '<i4'), ('left', '<i4'),
                ('side', '<i4'), ('factor', '<f4', 3), ('order', '<i4', 3), ('blur', '<i4'), ('ww', '<u4'), ('fw', '<u4'),
                ('reserved', '<i4')])
assert REC.itemsize == 96


def rotation_record(angle, w, h):
    """(mode, a0..a5) of Image.rotate(angle) on a w x h image (NEAREST, same canvas): Pillow's copy / transpose shortcuts,
    otherwise its affine matrix in 16.16 fixed point (Geometry.c ImagingTransformAffine)."""
    angle = angle % 360.0
    if angle == 0:
        return 1, (0,) * 6
    if angle == 180:
        return 2, (0,) * 6
    if angle in (90, 270) and w == h:
        return (3 if angle == 90 else 4), (0,) * 6
    rad = -math.radians(angle)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    if m[1] == 0 and m[3] == 0:
        # Pillow scales instead (ImagingScaleAffine) when sin rounds to 0 away from the shortcuts: |angle| < 3e-14 deg
        raise Mi355Error('augment: rotation by %r degrees takes a Pillow code path the device does not implement' % angle)
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return 0, (fix(m[0]), fix(m[1]), fix(m[0] * 0.5 + m[1] * 0.5 + m[2]), fix(m[3]), fix(m[4]), fix(m[3] * 0.5 + m[4] * 0.5 + m[5]))


def blur_record(radius, passes=3):
    """(on, ww, fw) of ImageFilter.GaussianBlur(radius): BoxBlur.c's box radius in float32 and its 24-bit weights.  The
    device implements integer box radius 0 (blur radius below ~1.4, the chain draws it from U(0, 0.8))."""
    if radius == 0:
        return 0, 0, 0
    f32 = np.float32
    sigma2 = f32(radius) * f32(radius) / f32(passes)
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * sigma2)
    fr = f32(l + a / (f32(6) * (sigma2 - (l + f32(1)) * (l + f32(1)))))
    if fr == 0:
        return 0, 0, 0
    if int(fr) != 0:
        raise Mi355Error('augment: blur radius %r needs a box radius >= 1, which the device path does not implement' % radius)
    ww = int(f32(1 << 24) / (fr * f32(2) + f32(1)))
    return 1, ww, ((1 << 24) - ww) // 2


def records(table, params):
    """Host records (numpy REC array) from the (B, 3) int64 (offset, h, w) table and the (B, 11) float64 parameters."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
    params = np.asarray(params, dtype=np.float64).reshape(-1, len(PARAM_COLUMNS))
    if len(table) != len(params):
        raise Mi355Error('augment: %d table rows for %d parameter rows' % (len(table), len(params)))
    rec = np.zeros(len(table), REC)
    for i, ((off, h, w), p) in enumerate(zip(table, params)):
        rec['offset'][i], rec['h'][i], rec['w'][i] = off, h, w
        rec['rot'][i], rec['a'][i] = rotation_record(float(p[0]), int(w), int(h))
        rec['top'][i], rec['left'][i], rec['side'][i] = int(p[1]), int(p[2]), int(p[3])
        rec['factor'][i] = p[4:7]
        rec['order'][i] = p[7:10]
        rec['blur'][i], rec['ww'][i], rec['fw'][i] = blur_record(float(p[10]))
    return rec


_ws = {}


def _workspace(device, B, S):
    n = int(load().mi355_augment_workspace(B, S))
    buf = _ws.get(device)
    if buf is None or buf.numel() < n:
        buf = _ws[device] = torch.empty(n, dtype=torch.uint8, device=device)
    return buf


def _prepare(name, packed_u8, table, params, out, size):
    """The argument contract augment and resize_normalize share: (packed, records on the host (pinned) and on the device,
    out (B, 3, size, size) fp32)."""
    if not (torch.is_tensor(packed_u8) and packed_u8.is_cuda and packed_u8.dtype == torch.uint8):
        raise Mi355Error('%s: the packed sources must be a uint8 CUDA tensor (no CPU path)' % name)
    packed_u8 = packed_u8.contiguous()
    dev = packed_u8.device
    table = table.numpy() if torch.is_tensor(table) else table
    params = params.numpy() if torch.is_tensor(params) else params
    rec = records(table, params)
    B = len(rec)
    if out is None:
        out = torch.empty(B, 3, size, size, dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (B, 3, size, size) or out.dtype != torch.float32 or out.device != dev
          or not out.is_contiguous()):
        raise Mi355Error('%s: out must be a contiguous fp32 (%d, 3, %d, %d) tensor on %s' % (name, B, size, size, dev))
    rec_host = torch.from_numpy(rec.view(np.uint8)).pin_memory()
    rec_dev = rec_host.to(dev, non_blocking=True)
    return packed_u8, rec_host, rec_dev, out


def augment(packed_u8, table, params, out=None, want_ema=False, size=256, mean=MEAN, std=STD):
    """packed_u8: flat uint8 CUDA tensor of the HWC RGB sources; table: (B, 3) (offset, h, w) and params: (B, 11)
    (``PARAM_COLUMNS``), both host tensors / arrays.  Returns x (B, 3, size, size) fp32 -- written into `out` when given --
    and, with want_ema, (x, image_ema).  size: a multiple of 16 up to 512."""
    packed_u8, rec_host, rec_dev, out = _prepare('augment', packed_u8, table, params, out, size)
    B, dev = out.shape[0], out.device
    ema = torch.empty(B, 3, size, size, dtype=torch.float32, device=dev) if want_ema else None
    ws = _workspace(dev, B, size)
    norm = np.array(list(mean) + list(std), dtype=np.float32)
    call('mi355_augment', ptr(packed_u8), packed_u8.numel(), rec_host.data_ptr(), ptr(rec_dev), B, size,
         norm.ctypes.data, ptr(out), ptr(ema), ptr(ws), ws.numel(), stream_ptr())
    return (out, ema) if want_ema else out


def resize_normalize(packed_u8, table, params, out=None, size=256, mean=MEAN, std=STD):
    """The geometry stage of ``augment`` alone (``mi355_resize_normalize``, one launch, no workspace): what ``augment`` returns
    as image_ema for the same arguments.  With the identity rows of ``DeviceResize`` (angle 0, the whole image as the crop)
    it is the validation chain Resize -> ToTensor -> Normalize, bit-identical with Pillow.  Same arguments and errors as
    ``augment``; returns x (B, 3, size, size) fp32, written into `out` when given."""
    packed_u8, rec_host, rec_dev, out = _prepare('resize_normalize', packed_u8, table, params, out, size)
    norm = np.array(list(mean) + list(std), dtype=np.float32)
    call('mi355_resize_normalize', ptr(packed_u8), packed_u8.numel(), rec_host.data_ptr(), ptr(rec_dev), out.shape[0], size,
         norm.ctypes.data, ptr(out), stream_ptr())
    return out
