"""Cost of the coordinate loss ("Coordinate loss"): the `mi355_coord_heatmap` launch on its own at B = 64,
K = 21, 64 x 64 heat-maps -- its time, its algorithmic bytes (the maps read once, the gradient written once) and, on the same box
in alternating rounds, `mi355_kl_heatmap` on the same tensor (which reads a second tensor, the labels) -- and graph replay of the
ResNet-50 iteration with an EMATeacher attached, the term off against `source` and `both`, alternating blocks of replays of
otherwise identical trainings in one process.  Prints one line per figure and, last, one JSON line with all of them.  Nothing
is asserted.

    python profiles/coord_cost.py [--arch resnet50] [-b 64] [--rounds 5] [--block 10] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

import torch

import mi355
import uda.model as models
from mi355 import ops
from mi355.da_step import CoordRegression, build_training
from mi355.optim import EMATeacher
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
from utils.synthetic import make_batch


def training(arch, dev, mode):
    torch.manual_seed(1)
    mk = lambda cls: (lambda bb: cls(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True))(
        models.__dict__[arch](pretrained=False)).to(dev)
    model = mk(PoseResNetx9)
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    teacher = mk(PoseResNetx10)
    teacher.load_state_dict(model.state_dict())
    step.ema = EMATeacher(model, teacher, opts, 0.999)
    if mode != 'off':
        step.coord = CoordRegression(target='teacher' if mode == 'both' else 'off', ema=step.ema)
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


def kernel_figures(dev, B, K, H, reps):
    g = torch.Generator(device='cpu').manual_seed(0)
    pred = (torch.randn(B, K, H, H, generator=g) * 3).to(dev)
    label = torch.randn(B, K, H, H, generator=g).abs().to(dev)
    coord = (torch.rand(B, K, 2, generator=g) * H).to(dev)
    w = (torch.rand(B, K, 1, generator=g) > 0.2).float().to(dev)
    n = pred.numel()
    res = {'B': B, 'K': K, 'heatmap': H, 'reps': reps,
           'coord_bytes': 8.0 * n + 24.0 * B * K,                 # maps read once + gradient written once + coord, weight, rows, uv
           'kl_bytes': 12.0 * n + 8.0 * B * K}                    # prediction and labels read + gradient written
    # (every call allocates its outputs through the caching allocator, as the training step does: both sides alike)
    fns = {'coord_grad': lambda: ops.coord_heatmap(pred, coord, w, 1.0, 1.0, 1.0, True),
           'coord_fwd': lambda: ops.coord_heatmap(pred, coord, w, 1.0, 1.0, 1.0, False),
           'kl_grad': lambda: ops.kl_heatmap(pred, label, w, 0.0, True, 1.0),
           'softargmax': lambda: ops.softargmax(pred, 1.0, 1.0)}
    rounds = {k: [] for k in fns}
    for _ in range(5):                                            # alternating rounds; the median round is reported
        for k, fn in fns.items():
            rounds[k].append(timed(fn, reps))
    for k, v in rounds.items():
        res[k + '_ms'], res[k + '_ms_rounds'] = statistics.median(v), v
    res['coord_grad_TBps'] = res['coord_bytes'] / res['coord_grad_ms'] / 1e9
    res['kl_grad_TBps'] = res['kl_bytes'] / res['kl_grad_ms'] / 1e9
    print('coord_heatmap + gradient B=%d K=%d %dx%d: %.4f ms (rounds %s), %.1f MB algorithmic, %.2f TB/s' % (
        B, K, H, H, res['coord_grad_ms'], ' '.join('%.4f' % x for x in rounds['coord_grad']), res['coord_bytes'] / 1e6, res['coord_grad_TBps']))
    print('coord_heatmap without the gradient: %.4f ms; softargmax alone: %.4f ms' % (res['coord_fwd_ms'], res['softargmax_ms']))
    print('kl_heatmap + gradient on the same box: %.4f ms (rounds %s), %.1f MB algorithmic, %.2f TB/s' % (
        res['kl_grad_ms'], ' '.join('%.4f' % x for x in rounds['kl_grad']), res['kl_bytes'] / 1e6, res['kl_grad_TBps']))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--skip-replay', action='store_true', help='the kernel only')
    ap.add_argument('--json', default=None, help='also write the result line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')
    res = {'kernel': kernel_figures(dev, a.b, 21, a.size // 4, a.reps)}
    if not a.skip_replay:
        batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev, with_keypoints=True)
        batch['x_t_ema'] = batch['x_t'].clone()
        steps = {k: training(a.arch, dev, k) for k in ('off', 'source', 'both')}
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
            print('coord %-6s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (
                k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
        for k in ('source', 'both'):
            rep[k + '_minus_off_ms'] = rep[k + '_ms'] - rep['off_ms']
            print('%s: %+.3f ms over off (%+.1f %%)' % (k, rep[k + '_minus_off_ms'], 100 * rep[k + '_minus_off_ms'] / rep['off_ms']))
        res['replay'] = rep
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
