"""Cost of the EMA teacher update: graph replay of the ResNet-50 iteration at B = 64, 256x256, with an
EMATeacher attached and without, alternating blocks of replays of two otherwise identical trainings in one process; and the
achieved bandwidth of the flat launch over the largest FusedSGD group (12 bytes per parameter: read e, read p, write e).

    python profiles/ema_cost.py [--arch resnet50] [-b 64] [--rounds 6] [--block 20]
"""
import argparse
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
from mi355.da_step import build_training
from mi355.optim import EMATeacher
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
from utils.synthetic import make_batch


def training(arch, dev, with_ema):
    torch.manual_seed(1)
    mk = lambda cls: (lambda bb: cls(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True))(
        models.__dict__[arch](pretrained=False)).to(dev)
    model = mk(PoseResNetx9)
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if with_ema:
        teacher = mk(PoseResNetx10)
        teacher.load_state_dict(model.state_dict())
        step.ema = EMATeacher(model, teacher, opts, 0.999)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--block', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')
    batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev)
    steps = {k: training(a.arch, dev, k == 'ema') for k in ('plain', 'ema')}
    for s in steps.values():
        for _ in range(3):
            s.run(batch)
        s.capture(batch, warmup=0)
        for _ in range(5):
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
    for k, v in ms.items():
        print('%-5s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
    print('difference of the medians: %.3f ms' % (statistics.median(ms['ema']) - statistics.median(ms['plain'])))

    ema = steps['ema'].ema
    print('launches per update: %d flat + %d batched (%d records)' % (len(ema._flat), ema._table is not None, ema._table[1] if ema._table else 0))
    E, P = max(ema._flat, key=lambda ep: ep[0].numel())
    n = E.numel()
    for _ in range(5):
        ops.ema_update(E, P, ema.coef)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 50
    ev[0].record()
    for _ in range(reps):
        ops.ema_update(E, P, ema.coef)
    ev[1].record()
    torch.cuda.synchronize()
    t = ev[0].elapsed_time(ev[1]) / reps
    print('flat launch, %d parameters (%.1f MB moved): %.4f ms back to back, %.2f TB/s' % (n, 12 * n / 1e6, t, 12 * n / t / 1e9))
    total = sum(e.numel() for e, _ in ema._flat)
    print('all flat groups: %d parameters, %.1f MB per update' % (total, 12 * total / 1e6))


if __name__ == '__main__':
    main()
