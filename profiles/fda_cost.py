"""Cost of the Fourier-domain stylisation: the launch pair of `mi355_fda_transfer` on its own at B = 64,
3 x 256 x 256 and beta in {0.01, 0.05, 0.09} -- each launch from the in-library launch log, the pair between device events,
the bytes it moves and its fp64 FMA count -- against the published full-FFT form written with torch.fft on the same tensors, and
graph replay of the ResNet-50 iteration with `fda` off against on at the smallest and the largest of those bands, alternating
blocks of replays of otherwise identical trainings in one process.  Prints one line per figure and, last, one JSON line with all
of them.

    python profiles/fda_cost.py [--arch resnet50] [-b 64] [--rounds 5] [--block 10] [--json PATH]
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
from mi355.augment import MEAN, STD
from mi355.da_step import FourierStyle, build_training
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.synthetic import make_batch

BETAS = (0.01, 0.05, 0.09)


def training(arch, dev, beta):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=64, fda=None if beta is None else FourierStyle(beta))
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
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


def torch_full_fft(x_s, x_t, b, mean, std):
    """The published form (fft2 -> fftshift -> swap the centre window of the amplitude -> ifftshift -> ifft2 -> real) on the
    de-normalised planes, re-normalised at the end; complex64, as torch.fft takes fp32 images."""
    p_s, p_t = x_s * std + mean, x_t * std + mean
    f_s, f_t = torch.fft.fft2(p_s), torch.fft.fft2(p_t)
    a_s, ph, a_t = torch.abs(f_s), torch.angle(f_s), torch.abs(f_t)
    a_s, a_t = torch.fft.fftshift(a_s, dim=(-2, -1)), torch.fft.fftshift(a_t, dim=(-2, -1))
    ch, cw = x_s.shape[-2] // 2, x_s.shape[-1] // 2
    a_s[..., ch - b:ch + b + 1, cw - b:cw + b + 1] = a_t[..., ch - b:ch + b + 1, cw - b:cw + b + 1]
    a_s = torch.fft.ifftshift(a_s, dim=(-2, -1))
    out = torch.fft.ifft2(torch.polar(a_s, ph)).real
    return (out - mean) / std


def kernel_figures(dev, B, S, reps):
    g = torch.Generator(device='cpu').manual_seed(0)
    mean, std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    x_s = ((torch.rand(B, 3, S, S, generator=g).to(dev) - mean) / std).contiguous()
    x_t = ((torch.rand(B, 3, S, S, generator=g).to(dev) ** 2 - mean) / std).contiguous()
    res = {'B': B, 'image': S, 'reps': reps, 'bands': {}}
    for beta in BETAS:
        b = ops.fda_band(S, S, beta)
        need = mi355.load().mi355_fda_workspace_bytes(B, 3, S, S, b)
        out, ws = torch.empty_like(x_s), torch.empty(need, dtype=torch.uint8, device=dev)
        call = lambda: ops.fda_transfer(x_s, x_t, beta, out=out, ws=ws)
        rounds = {'pair': [], 'torch': []}
        for _ in range(5):                            # alternating, so that clocks and neighbours hit both alike
            rounds['pair'].append(timed(call, reps))
            rounds['torch'].append(timed(lambda: torch_full_fft(x_s, x_t, b, mean, std), max(reps // 5, 3), warm=2))
        torch.cuda.synchronize()
        ops.prof_reset(); ops.prof_enable(2)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        log = ops.prof_launches()
        ops.prof_enable(0); ops.prof_reset()
        each = {k: statistics.median(e['us'] for e in log if e['label'].startswith('fda ' + k)) for k in ('spectrum', 'apply')}
        fmas = sum(e['flops'] for e in log[:2]) / 2.0
        px = float(x_s.numel())
        nbytes = 4.0 * 4.0 * px + 2.0 * need          # three reads and one write of the images, the partials written and read once
        worst = float((out - torch_full_fft(x_s, x_t, b, mean, std)).abs().max())
        r = {'b': b, 'ws_bytes': need, 'pair_ms': statistics.median(rounds['pair']), 'pair_ms_rounds': rounds['pair'],
             'torch_ms': statistics.median(rounds['torch']), 'torch_ms_rounds': rounds['torch'], 'spectrum_us': each['spectrum'],
             'apply_us': each['apply'], 'bytes': nbytes, 'fp64_fmas': fmas, 'max_abs_diff_to_torch_complex64': worst}
        r['TBps'] = nbytes / r['pair_ms'] / 1e9
        r['fp64_TFMAps'] = fmas / r['pair_ms'] / 1e9
        r['torch_over_pair'] = r['torch_ms'] / r['pair_ms']
        res['bands'][str(beta)] = r
        print('fda_transfer B=%d %dx%d beta=%g (b=%d): pair %.4f ms (rounds %s; spectrum %.1f us, apply %.1f us), %.1f MB -> %.2f TB/s, '
              '%.3g fp64 FMAs -> %.2f TFMA/s' % (B, S, S, beta, b, r['pair_ms'], ' '.join('%.4f' % x for x in rounds['pair']), each['spectrum'],
                                                 each['apply'], nbytes / 1e6, r['TBps'], fmas, r['fp64_TFMAps']))
        print('  the full-FFT torch expression on the same tensors: %.4f ms (%.1fx); largest difference to it %.2e (complex64)'
              % (r['torch_ms'], r['torch_over_pair'], worst))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--skip-replay', action='store_true', help='the launch pair only')
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
        steps = {k: training(a.arch, dev, beta) for k, beta in (('off', None), ('on_0.01', 0.01), ('on_0.09', 0.09))}
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
            print('fda %-8s replay: median %.3f ms / iteration, %d graphs  (blocks of %d: %s)' % (
                k, statistics.median(v), len(steps[k].graphs), a.block, ' '.join('%.3f' % x for x in v)))
        for k in ('on_0.01', 'on_0.09'):
            rep[k + '_minus_off_ms'] = rep[k + '_ms'] - rep['off_ms']
            print('%s: %+.3f ms over off (%.2f %%)' % (k, rep[k + '_minus_off_ms'], 100 * rep[k + '_minus_off_ms'] / rep['off_ms']))
        res['replay'] = rep
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
