"""Cost of the in-graph gradient-norm clipping ("Gradient clipping and step guard"): graph replay of the
ResNet-50 iteration at B = 64, 256x256, bf16 with the clipper off against on (max_norm = 1), alternating blocks of replays of two
otherwise identical trainings in one process; then the two launches of one measurement (mi355_grad_sumsq_batched +
mi355_grad_clip_coef) on their own over the flat gradient buffers of that training -- update A's ranges (the backbone, the neck and
the four heads) and update C's (backbone and neck) -- with the rate at which they read the gradients.

    python profiles/gradclip_cost.py [--arch resnet50] [-b 64] [--rounds 6] [--block 20] [--max-norm 1.0]
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
from mi355.optim import GradClipper
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.synthetic import make_batch


def timed(fn, inner=20, reps=10):
    """Microseconds per call of `fn`, from replays of a graph that holds `inner` calls (eager launches of kernels this short
    would time the host)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with mi355.no_gc_in_capture():
        with torch.cuda.graph(g, capture_error_mode=mi355.graph_capture_mode()):
            for _ in range(inner):
                fn()
    for _ in range(2):
        g.replay()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        g.replay()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / (reps * inner) * 1e3


def training(arch, dev, max_norm):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if max_norm is not None:
        step.clip = GradClipper(max_norm, dev)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--block', type=int, default=20)
    ap.add_argument('--max-norm', type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')

    # ---- the iteration in graph replay, off against on
    batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev)
    steps = {k: training(a.arch, dev, a.max_norm if k == 'on' else None) for k in ('off', 'on')}
    for st in steps.values():
        for _ in range(3):
            st.run(batch)
        st.capture(batch, warmup=0)
        for _ in range(5):
            st.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, st in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                st.replay()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.block * 1e3)
    for k, v in ms.items():
        print('clip %-3s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
    print('difference of the medians: %.3f ms' % (statistics.median(ms['on']) - statistics.median(ms['off'])))
    on = steps['on']
    norms, skipped = on.clip.read()
    print('last replay: ' + '  '.join('%s norm %.4g coef %.4g skip %d' % ((s,) + norms[s]) for s in on.clip.SLOTS) + '  skipped steps: %d' % skipped)

    # ---- the two launches of one measurement on their own, over the gradients that training left in its flat buffers
    for slot, keys in (('a', ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3')), ('c', ('f',))):
        opts = [on.opt[k] for k in keys]
        spare = GradClipper(a.max_norm, dev)
        spare.measure(opts, slot)
        t = spare._tables[slot]
        n = sum(hi - lo for _, lo, hi in t['sig'])
        us = timed(lambda: spare.measure(opts, slot))
        print('measurement of update %s: %d ranges, %d floats (%.1f MB), %d blocks: %.1f us for the two launches (graph replay), %.2f TB/s'
              % (slot.upper(), t['count'], n, n * 4 / 1e6, t['blocks'], us, n * 4 / us / 1e6))
        one = timed(lambda: ops.grad_clip_coef(t['partials'], t['blocks'], spare.record(slot)))
        print('  of which mi355_grad_clip_coef over %d partial sums: %.1f us' % (t['blocks'], one))


if __name__ == '__main__':
    main()
