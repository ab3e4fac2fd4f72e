"""Cost of the adaptive occlusion and the teacher-confidence gate: the three launches of csrc/occlude.hip on
their own -- `mi355_occlude_images` at B = 64, 3 x 256 x 256 with N = 1 and N = 8 beside `mi355_mirror_batch` and
`mi355_mixup_pairs` on the same tensors, `mi355_peak_prob` at 1344 maps of 64 x 64 beside `mi355_argmax2d` and `mi355_softargmax`,
`mi355_teacher_select` -- each between device events and from the in-library launch log, with the bytes it moves; and graph
replay of the ResNet-50 iteration with `--mt-loss on`: plain, with `--occlude keypoint` (threshold 0: every finite map is a candidate,
so boxes are drawn) and with `--teacher-conf` alone (the threshold at the median of the peaks the teacher's first forward gives, so
about half of the maps pass; the teacher's decay is 1 in all three, so that its peaks stay where the threshold was put), alternating blocks of replays of otherwise identical trainings in one process; the share of
confident maps and the boxes per sample of the last replay are reported with the times.  Prints one line per figure and, last,
one JSON line with all.

    python profiles/occlude_cost.py [--arch resnet50] [-b 64] [--rounds 5] [--block 10] [--json PATH]
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
from mi355.optim import EMATeacher
from mi355.teacher import KeypointOcclusion, MeanTeacher
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9, PoseResNetx10
from utils.synthetic import make_batch

def median_threshold(y):
    """Between the two middle neighbours of the sorted peaks of softmax(y) of the maps y (B, K, H, W): their geometric mean."""
    p = ops.peak_prob(y.detach().float().contiguous(), 1.0)[2].double().view(-1).sort().values
    k = p.numel() // 2
    return float((p[k - 1] * p[k]).sqrt())


def training(arch, dev, kind, tau=0.0):
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
    # decay 1: the update launches run, the teacher stays where it is -- on the one synthetic batch its maps, and with them the share
    # of maps that pass a threshold, are then the same in every replay (the student's noise-image predictions collapse otherwise,
    # and the teacher's peaks follow them below any threshold chosen beforehand)
    step.ema = EMATeacher(model, teacher, opts, 1.0, warmup=False)
    step.mt = MeanTeacher(step.ema, weight=0.1, k='all')
    if kind == 'occlude':
        step.occlude = KeypointOcclusion(prob=0.5, n=1, size=(0.08, 0.16), seed=1)
    if kind == 'conf':
        step.teacher_conf = float(tau)
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


def kernel_figures(dev, B, S, reps):
    g = torch.Generator(device='cpu').manual_seed(0)
    K, h = 21, S // 4
    x = torch.randn(B, 3, S, S, generator=g).to(dev)
    x2 = torch.randn(B, 3, S, S, generator=g).to(dev)
    y = torch.rand(B, K, h, h, generator=g).to(dev)
    y2 = torch.rand(B, K, h, h, generator=g).to(dev)
    w_in = torch.ones(B, K, 1, device=dev)
    lam = torch.full((B,), 0.7, device=dev)
    out_x = torch.empty_like(x)
    mir = torch.empty(2 * B, 3, S, S, device=dev)
    mix = (torch.empty(2 * B, 3, S, S, device=dev), torch.empty(2 * B, K, h, h, device=dev), torch.empty(2 * B, K, 1, device=dev))
    # boxes as teacher_select draws them at prob = 1: one and eight per sample
    sel = {}
    for n in (1, 8):
        o = KeypointOcclusion(prob=1.0, n=n, size=(0.08, 0.16), seed=0)
        o.draw(B, dev)
        o.select(y, 0.0, S, w_in=w_in)
        sel[n] = o
    o8 = sel[8]
    peak_out = (torch.empty(B, K, dtype=torch.int32, device=dev), torch.empty(B, K, 2, device=dev), torch.empty(B, K, device=dev))
    lo, hi = o8.sides(S)
    sel_out = (o8.conf, o8.w_out, o8.boxes, o8.count)
    o1 = sel[1]
    sel_out1 = (o1.conf, o1.w_out, o1.boxes, o1.count)
    nx, ny = float(x.numel()), float(y.numel())
    calls = {
        'occlude_images_n1': (lambda: ops.occlude_images(x, sel[1].boxes, out=out_x), 8.0 * nx + 16.0 * B),
        'occlude_images_n8': (lambda: ops.occlude_images(x, sel[8].boxes, out=out_x), 8.0 * nx + 128.0 * B),
        'mirror_batch': (lambda: mi355.call('mi355_mirror_batch', x.data_ptr(), mir.data_ptr(), B, 3, S, S, mi355.stream_ptr()), 12.0 * nx),
        'mixup_pairs': (lambda: ops.mixup_pairs(x, y, w_in, x2, y2, w_in, lam, out=mix), 16.0 * (nx + ny + B * K) + 4.0 * B),
        'peak_prob': (lambda: ops.peak_prob(y, 1.0, out=peak_out), 4.0 * ny + 16.0 * B * K),
        'argmax2d': (lambda: ops.argmax2d(y), 4.0 * ny + 16.0 * B * K),
        'softargmax': (lambda: ops.softargmax(y, 1.0, 1.0), 4.0 * ny + 8.0 * B * K),
        'teacher_select_n8': (lambda: ops.teacher_select(o8.p, o8.xy, o8.u, 0.0, 1.0, 8, lo, hi, S, (h, h), w_in=w_in, out=sel_out, stats=o8.stats),
                              24.0 * B * K + 20.0 * B * 8),
        'teacher_select_n1': (lambda: ops.teacher_select(o1.p, o1.xy, o1.u, 0.0, 1.0, 1, lo, hi, S, (h, h), w_in=w_in, out=sel_out1, stats=o1.stats),
                              24.0 * B * K + 20.0 * B),
        'teacher_select_n0': (lambda: ops.teacher_select(o1.p, tau=0.0, n=0, w_in=w_in, out=(o1.conf, o1.w_out, None, None), stats=o1.stats),
                              16.0 * B * K),
    }
    rounds = {k: [] for k in calls}
    for _ in range(5):                                    # alternating, so that clocks and neighbours hit all alike
        for k, (fn, _) in calls.items():
            rounds[k].append(timed(fn, reps, warm=3))
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(2)
    for _ in range(10):
        for k in ('occlude_images_n1', 'occlude_images_n8', 'peak_prob', 'mirror_batch'):
            calls[k][0]()
    torch.cuda.synchronize()
    log = ops.prof_launches()
    ops.prof_enable(0); ops.prof_reset()
    res = {'B': B, 'image': S, 'heatmap': h, 'K': K, 'reps': reps, 'calls': {},
           'boxes_per_sample': {n: float(sel[n].count.float().mean()) for n in sel},
           'blanked_fraction': {n: float((ops.occlude_images(x, sel[n].boxes) != x).float().mean()) for n in sel}}
    for k, (fn, nbytes) in calls.items():
        ms = statistics.median(rounds[k])
        r = {'ms': ms, 'ms_rounds': rounds[k], 'bytes': nbytes, 'TBps': nbytes / ms / 1e9}
        word = k.split('_n')[0]
        us = [e['us'] for e in log if e['label'].split()[0] == word and not k.startswith('teacher') and
              (not k.startswith('occlude') or e['label'].split()[2] == 'N' + k[-1])]
        if us:
            r['launch_log_us'] = statistics.median(us)
        res['calls'][k] = r
        print('%-22s %.4f ms (rounds %s)%s, %.1f MB -> %.2f TB/s' % (k, ms, ' '.join('%.4f' % v for v in rounds[k]),
              (', launch log %.1f us' % r['launch_log_us']) if us else '', nbytes / 1e6, r['TBps']))
    c = res['calls']
    res['occlude_n1_over_mirror_bytes_per_s'] = c['occlude_images_n1']['TBps'] / c['mirror_batch']['TBps']
    res['occlude_n8_over_mirror_bytes_per_s'] = c['occlude_images_n8']['TBps'] / c['mirror_batch']['TBps']
    res['peak_prob_over_argmax_plus_softargmax'] = c['peak_prob']['ms'] / (c['argmax2d']['ms'] + c['softargmax']['ms'])
    print('occlude_images bytes / s over mirror_batch: N = 1 %.2f, N = 8 %.2f; peak_prob over argmax2d + softargmax: %.2f'
          % (res['occlude_n1_over_mirror_bytes_per_s'], res['occlude_n8_over_mirror_bytes_per_s'], res['peak_prob_over_argmax_plus_softargmax']))
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
        steps = {k: training(a.arch, dev, k) for k in ('plain', 'occlude')}
        steps['plain'].run(batch)                         # the teacher's first forward: where the peaks of this run lie
        p0 = ops.peak_prob(steps['plain'].out['y_t_ema'].detach().float().contiguous(), 1.0)[2]
        tau = median_threshold(steps['plain'].out['y_t_ema'])
        steps['conf'] = training(a.arch, dev, 'conf', tau)
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
        rep = {'arch': a.arch, 'block': a.block, 'occlude_tau': 0.0, 'conf_tau': tau, 'flat_map_peak': 1.0 / (a.size // 4) ** 2,
               'first_forward_peaks_min_median_max': [float(p0.min()), float(p0.median()), float(p0.max())]}
        for k, v in ms.items():
            rep[k + '_ms'], rep[k + '_ms_blocks'] = statistics.median(v), v
            print('%-8s replay: median %.3f ms / iteration, %d graphs  (blocks of %d: %s)' % (
                k, statistics.median(v), len(steps[k].graphs), a.block, ' '.join('%.3f' % x for x in v)))
        rep['occlude_minus_plain_ms'] = rep['occlude_ms'] - rep['plain_ms']
        rep['conf_minus_plain_ms'] = rep['conf_ms'] - rep['plain_ms']
        rep['plain_spread_ms'] = max(ms['plain']) - min(ms['plain'])
        for k in ('occlude', 'conf'):
            o = steps[k].out
            rep[k + '_conf_share'] = float(o['conf_share'])
        rep['occlude_boxes_per_sample'] = float(steps['occlude'].out['occ_boxes'])
        if not (rep['occlude_boxes_per_sample'] > 0 and 0 < rep['conf_conf_share'] < 1):
            raise SystemExit('the feature did nothing in the timed runs (boxes / sample %r, conf share of the gated run %r): nothing to report'
                             % (rep['occlude_boxes_per_sample'], rep['conf_conf_share']))
        print('occlude (tau 0, boxes / sample %.2f, conf share %.2f): %+.3f ms over plain; teacher-conf alone (tau %.6f, conf share %.2f): '
              '%+.3f ms; spread of the plain blocks %.3f ms' % (rep['occlude_boxes_per_sample'], rep['occlude_conf_share'],
              rep['occlude_minus_plain_ms'], tau, rep['conf_conf_share'], rep['conf_minus_plain_ms'], rep['plain_spread_ms']))
        res['replay'] = rep
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
