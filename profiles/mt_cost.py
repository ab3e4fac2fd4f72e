"""Cost of the mean-teacher consistency term: graph replay of the ResNet-50 iteration at B = 64, 256x256
with an EMATeacher attached, `mt` off against on, alternating blocks of replays of two otherwise identical trainings in one
process; then the pieces on their own -- the teacher's folded eval forward, its refresh (fold + pack launches) and the loss.

    python profiles/mt_cost.py [--arch resnet50] [-b 64] [--rounds 6] [--block 20]
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
from mi355.da_step import build_training
from mi355.optim import EMATeacher
from mi355.teacher import MeanTeacher
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
from utils.synthetic import make_batch


def training(arch, dev, with_mt):
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
    if with_mt:
        step.mt = MeanTeacher(step.ema, weight=0.05)
    return step


def timed(fn, reps):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


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
    batch['x_t_ema'] = batch['x_t'].clone()
    steps = {k: training(a.arch, dev, k == 'on') for k in ('off', 'on')}
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
        print('mt %-3s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
    print('difference of the medians: %.3f ms' % (statistics.median(ms['on']) - statistics.median(ms['off'])))

    mt = steps['on'].mt
    it = mt.teacher
    n = sum(it._n)
    print('teacher: %d folded (conv, BatchNorm) pairs, %d weights; refresh = 1 fold + %d batched pack + %d stem pack launches'
          % (len(it._pairs), n, len(it._packs), len(it._stem)))
    x = batch['x_t_ema']
    print('teacher eval forward, %d images, eager launches back to back: %.3f ms' % (a.b, timed(lambda: it.forward(x), 20)))
    t = timed(it.refresh, 50)
    print('refresh (fold + pack + plain repack): %.4f ms, %.2f TB/s over 8 + 6 bytes per folded weight' % (t, 14 * n / t / 1e9))
    with torch.no_grad():
        y = it.forward(x).clone()
    p = torch.randn_like(y).requires_grad_(True)
    print('loss forward (masked MSE + gradient, sum, scale) on %s: %.4f ms' % (tuple(y.shape), timed(lambda: mt.loss(p, y), 50)))


if __name__ == '__main__':
    main()
