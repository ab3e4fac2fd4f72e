"""Cost of the Adam / AdamW update ("Adam / AdamW"): graph replay of the ResNet-50 iteration at B = 64,
256x256, bf16 under --optimizer sgd, adam and adamw, alternating blocks of replays of three otherwise identical trainings in one
process; then the optimizer launches of update A (the backbone and the neck, and the four heads: five optimizers) and of update C
(backbone and neck) on their own, over the flat buffers those trainings left: mi355_adam_step_batched + mi355_adam_tick_batched per
optimizer against the mi355_sgd_nesterov launches over the same ranges, with the bytes per second each moves (Adam reads p, g, m, v
and writes p, m, v: 28 bytes per element; SGD reads p, g, buf and writes p, buf: 20).  Writes what it measured to a JSON file.

    python profiles/adam_cost.py [--arch resnet50] [-b 64] [--rounds 4] [--block 10] [--out profiles/adam_cost.json]
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
from mi355.da_step import build_training
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.synthetic import make_batch

KINDS = ('sgd', 'adam', 'adamw')
UPDATES = (('a', ('f', 'h', 'h_adv', 'h_adv2', 'h_adv3')), ('c', ('f',)))


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


def training(arch, dev, kind):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=64, optimizer=kind)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adam_cost.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')
    result = dict(arch=a.arch, batch=a.b, size=a.size, dtype='bf16', device=torch.cuda.get_device_name(0), rounds=a.rounds, block=a.block)

    # ---- the iteration in graph replay under the three optimizers
    batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev)
    steps = {k: training(a.arch, dev, k) for k in KINDS}
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
    result['iteration_ms'] = {}
    for k, v in ms.items():
        print('%-5s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
        result['iteration_ms'][k] = dict(median=statistics.median(v), blocks=v)
    for k in ('adam', 'adamw'):
        print('%s - sgd, difference of the medians: %.3f ms' % (k, statistics.median(ms[k]) - statistics.median(ms['sgd'])))

    # ---- the optimizer launches of updates A and C on their own
    result['updates'] = {}
    for slot, keys in UPDATES:
        row = result['updates'][slot] = {}
        # Adam: two launches per optimizer over the tables the training built
        tables = [steps['adamw'].opt[k]._table for k in keys]
        n = sum(s[2] for t in tables for s in t['sig'])

        def adam():
            for t in tables:
                ops.adam_step_batched(t['table'], t['count'], t['blocks'])
                ops.adam_tick_batched(t['table'], t['count'])

        def adam_steps_only():
            for t in tables:
                ops.adam_step_batched(t['table'], t['count'], t['blocks'])

        us, us_step = timed(adam), timed(adam_steps_only)
        row['adam'] = dict(optimizers=len(tables), launches=2 * len(tables), items=sum(t['count'] for t in tables), blocks=sum(t['blocks'] for t in tables),
                           floats=n, bytes=28 * n, us=us, us_step_launches=us_step, us_per_launch=us / (2 * len(tables)), bytes_per_s=28 * n / (us * 1e-6))
        print('update %s, adam: %d optimizers, %d parameters, %d floats (%.1f MB moved): %.1f us for %d launches (%.1f us in the step '
              'launches), %.2f TB/s' % (slot.upper(), len(tables), row['adam']['items'], n, 28 * n / 1e6, us, 2 * len(tables), us_step, 28 * n / us / 1e6))
        # SGD: one launch per flat group over the same ranges
        groups = [(f, steps['sgd'].opt[k].param_groups[f['gi']]) for k in keys for f in steps['sgd'].opt[k]._flat if f is not None]
        n_sgd = sum(f['P'].numel() for f, _ in groups)

        def sgd():
            for f, g in groups:
                ops.sgd_nesterov(f['P'], f['G'], f['M'], f['lr_dev'], g['momentum'], g['weight_decay'], g['nesterov'])

        us = timed(sgd)
        row['sgd'] = dict(launches=len(groups), floats=n_sgd, bytes=20 * n_sgd, us=us, us_per_launch=us / len(groups), bytes_per_s=20 * n_sgd / (us * 1e-6))
        print('update %s, sgd:  %d launches, %d floats (%.1f MB moved): %.1f us, %.2f TB/s' % (slot.upper(), len(groups), n_sgd, 20 * n_sgd / 1e6, us, 20 * n_sgd / us / 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote ' + a.out)


if __name__ == '__main__':
    main()
