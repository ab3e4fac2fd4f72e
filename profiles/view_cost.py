"""Cost of the geometric teacher view: the two warp launches and `mi355_mse_heatmap_w` on their own at
B = 64, 3 x 256 x 256 images and 21 x 64 x 64 heat-maps -- each between device events and from the in-library launch log, with the
bytes it moves -- against `affine_grid` + `grid_sample` plus the mask written in torch on the same tensors, with
`mi355_mirror_batch` and `mi355_mixup_pairs` beside them as streaming references; and graph replay of the ResNet-50 iteration with
`--mt-loss on`, view `same` against `geom`, alternating blocks of replays of otherwise identical trainings in one process.  Prints
one line per figure and, last, one JSON line with all of them.

    python profiles/view_cost.py [--arch resnet50] [-b 64] [--rounds 5] [--block 10] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

import numpy as np
import torch

import mi355
import uda.model as models
from mi355 import ops
from mi355.da_step import build_training
from mi355.optim import EMATeacher
from mi355.teacher import GeometricView, MeanTeacher
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
from utils.synthetic import make_batch

VIEW = dict(rot_deg=30.0, scale=(0.75, 1.25), shift=0.1, margin=2)


def training(arch, dev, view):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    eb = models.__dict__[arch](pretrained=False)
    teacher = PoseResNetx10(eb, Upsampling(eb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    teacher.load_state_dict(model.state_dict(), strict=False)
    for p in teacher.parameters():
        p.requires_grad = False
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    step.ema = EMATeacher(model, teacher, opts, 0.999, warmup=False)
    step.mt = MeanTeacher(step.ema, weight=0.1, k='all')
    if view:
        step.view = GeometricView(seed=1, **VIEW)
    return step


def timed(fn, reps, warm=5):
    """Mean GPU time per call in ms: `reps` calls back to back between two events, after `warm` unmeasured ones."""
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def torch_warp(x, theta):
    """The yardstick: affine_grid + grid_sample (bilinear, zeros, align_corners=True) with the matrix in normalised coordinates."""
    grid = torch.nn.functional.affine_grid(theta, list(x.shape), align_corners=True)
    return torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def normalised(m, H, W):
    """A pixel-space 2 x 3 matrix (B, 2, 3) acting on (x, y, 1) as affine_grid's theta acting on coordinates in [-1, 1]."""
    m = m.astype(np.float64)
    sx, sy = (W - 1) / 2.0, (H - 1) / 2.0
    out = np.empty_like(m)
    out[:, 0, 0], out[:, 0, 1] = m[:, 0, 0], m[:, 0, 1] * sy / sx
    out[:, 1, 0], out[:, 1, 1] = m[:, 1, 0] * sx / sy, m[:, 1, 1]
    out[:, 0, 2] = (m[:, 0, 0] * sx + m[:, 0, 1] * sy + m[:, 0, 2]) / sx - 1.0
    out[:, 1, 2] = (m[:, 1, 0] * sx + m[:, 1, 1] * sy + m[:, 1, 2]) / sy - 1.0
    return out.astype(np.float32)


def torch_unwarp(y, theta, theta_inv, margin, w_in):
    """grid_sample plus the flag: arg-max, the margin test and the pre-image test, in torch."""
    B, K, h, w = y.shape
    out = torch_warp(y, theta)
    idx = y.view(B, K, -1).argmax(dim=2)
    ux, uy = (idx % w).float(), torch.div(idx, w, rounding_mode='floor').float()
    ok = (ux >= margin) & (ux <= w - 1 - margin) & (uy >= margin) & (uy <= h - 1 - margin)
    px = theta_inv[:, 0, 0, None] * ux + theta_inv[:, 0, 1, None] * uy + theta_inv[:, 0, 2, None]
    py = theta_inv[:, 1, 0, None] * ux + theta_inv[:, 1, 1, None] * uy + theta_inv[:, 1, 2, None]
    ok = ok & (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    valid = ok.float()
    return out, valid, w_in * valid.view_as(w_in)


def kernel_figures(dev, B, S, reps):
    g = torch.Generator(device='cpu').manual_seed(0)
    K, h = 21, S // 4
    x = torch.randn(B, 3, S, S, generator=g).to(dev)
    x2 = torch.randn(B, 3, S, S, generator=g).to(dev)
    y = torch.rand(B, K, h, h, generator=g).to(dev)
    y2 = torch.rand(B, K, h, h, generator=g).to(dev)
    w_in = torch.ones(B, K, 1, device=dev)
    view = GeometricView(seed=0, **VIEW)
    view.draw(B, dev, image_size=S, heatmap_size=h)
    recs, host = view.recs, view.recs_host.reshape(B, 3, 2, 3)
    th_img = torch.from_numpy(normalised(host[:, 0], S, S)).to(dev)
    th_hm = torch.from_numpy(normalised(host[:, 1], h, h)).to(dev)
    inv_px = torch.from_numpy(host[:, 2].copy()).to(dev)
    rec = ops.mse_record((1 << K) - 1, 2.0 / y.numel(), device=dev)
    lam = torch.full((B,), 0.7, device=dev)
    out_x = torch.empty_like(x)
    out_u = (torch.empty_like(y), torch.empty(B, K, device=dev), torch.empty(B, K, 1, device=dev))
    rows, grad = torch.empty(B, K, device=dev), torch.empty_like(y)
    mir = torch.empty(2 * B, 3, S, S, device=dev)
    mix = (torch.empty(2 * B, 3, S, S, device=dev), torch.empty(2 * B, K, h, h, device=dev), torch.empty(2 * B, K, 1, device=dev))
    valid = out_u[1]
    nx, ny = float(x.numel()), float(y.numel())
    calls = {
        'affine_warp': (lambda: ops.affine_warp_images(x, recs, out=out_x), 8.0 * nx + 72.0 * B),
        'affine_unwarp': (lambda: ops.affine_unwarp_heatmaps(y, recs, 2.0, w_in=w_in, out=out_u), 8.0 * ny + 72.0 * B + 12.0 * B * K),
        'mse_heatmap_w': (lambda: ops.mse_heatmap_w(y, y2, rec, valid, True, rows=rows, grad=grad), 12.0 * ny + 4.0 * B * K),
        'mse_heatmap': (lambda: ops.mse_heatmap(y, y2, rec, True, rows=rows, grad=grad), 12.0 * ny),
        'mirror_batch': (lambda: mi355.call('mi355_mirror_batch', x.data_ptr(), mir.data_ptr(), B, 3, S, S, mi355.stream_ptr()), 12.0 * nx),
        'mixup_pairs': (lambda: ops.mixup_pairs(x, y, w_in, x2, y2, w_in, lam, out=mix), 16.0 * (nx + ny + B * K) + 4.0 * B),
        'torch_grid_sample_images': (lambda: torch_warp(x, th_img), 8.0 * nx),
        'torch_grid_sample_heatmaps_and_mask': (lambda: torch_unwarp(y, th_hm, inv_px, 2.0, w_in), 8.0 * ny),
        'torch_masked_mse': (lambda: (((y - y2) ** 2).sum(dim=(2, 3)) * valid, (y - y2) * valid.view(B, K, 1, 1)), 12.0 * ny),
    }
    ops.affine_unwarp_heatmaps(y, recs, 2.0, w_in=w_in, out=out_u)        # (valid holds flags before mse_heatmap_w reads it)
    rounds = {k: [] for k in calls}
    for _ in range(5):                                    # alternating, so that clocks and neighbours hit all alike
        for k, (fn, _) in calls.items():
            rounds[k].append(timed(fn, reps if not k.startswith('torch') else max(reps // 5, 3), warm=3))
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    for _ in range(10):
        for k in ('affine_warp', 'affine_unwarp', 'mse_heatmap_w'):
            calls[k][0]()
    torch.cuda.synchronize()
    log = ops.prof_launches()
    ops.prof_enable(0); ops.prof_reset()
    res = {'B': B, 'image': S, 'heatmap': h, 'K': K, 'reps': reps, 'valid_fraction': float(valid.mean()), 'calls': {}}
    # what the two forms disagree by (fp32 coordinates in pixels against normalised ones): reported, not a threshold
    res['max_abs_diff_images_to_grid_sample'] = float((ops.affine_warp_images(x, recs) - torch_warp(x, th_img)).abs().max())
    res['max_abs_diff_heatmaps_to_grid_sample'] = float((out_u[0] - torch_warp(y, th_hm)).abs().max())
    for k, (fn, nbytes) in calls.items():
        ms = statistics.median(rounds[k])
        r = {'ms': ms, 'ms_rounds': rounds[k], 'bytes': nbytes, 'TBps': nbytes / ms / 1e9}
        us = [e['us'] for e in log if e['label'].split()[0] == k]
        if us:
            r['launch_log_us'] = statistics.median(us)
        res['calls'][k] = r
        print('%-38s %.4f ms (rounds %s)%s, %.1f MB -> %.2f TB/s' % (k, ms, ' '.join('%.4f' % v for v in rounds[k]),
              (', launch log %.1f us' % r['launch_log_us']) if us else '', nbytes / 1e6, r['TBps']))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--skip-replay', action='store_true', help='the launches only')
    ap.add_argument('--json', default=None, help='also write the result line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')
    res = {'kernel': kernel_figures(dev, a.b, a.size, a.reps)}
    if not a.skip_replay:
        batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev)
        steps = {k: training(a.arch, dev, k == 'geom') for k in ('same', 'geom')}
        for s in steps.values():
            for _ in range(3):
                s.run(batch)
            s.capture(batch, warmup=0)
            for _ in range(3):
                s.replay()
        torch.cuda.synchronize()
        ms = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, s in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.block):
                    s.replay()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.block * 1e3)
        rep = {'arch': a.arch, 'block': a.block}
        for k, v in ms.items():
            rep[k + '_ms'], rep[k + '_ms_blocks'] = statistics.median(v), v
            print('view %-5s replay: median %.3f ms / iteration, %d graphs  (blocks of %d: %s)' % (
                k, statistics.median(v), len(steps[k].graphs), a.block, ' '.join('%.3f' % x for x in v)))
        rep['geom_minus_same_ms'] = rep['geom_ms'] - rep['same_ms']
        rep['same_spread_ms'] = max(ms['same']) - min(ms['same'])
        print('geom: %+.3f ms over same (%.2f %%); spread of the same blocks %.3f ms'
              % (rep['geom_minus_same_ms'], 100 * rep['geom_minus_same_ms'] / rep['same_ms'], rep['same_spread_ms']))
        res['replay'] = rep
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
