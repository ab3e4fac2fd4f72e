"""Cost of the MMD alignment term: the three mmd_ launches at B = 64 + 64, K = 21, 64 x 64 beside the
reference's torch expression (the n x n x HW broadcast, forward and backward through autograd) on the same GPU; then graph
replay of the ResNet-50 iteration at B = 64, 256x256, bf16 with `mmd` off against on, alternating blocks of replays of two
otherwise identical trainings in one process.

    python profiles/mmd_cost.py [--arch resnet50] [-b 64] [--rounds 6] [--block 20] [--skip-iteration]
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
from mi355.da_step import MMDAlign, build_training
from uda.model.loss import MMD_loss3
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.synthetic import make_batch


def torch_expression(source, target, kernel_mul=2.0, kernel_num=5):
    """MMD_loss3 as the reference writes it: per joint, the (n, n, HW) difference tensor, its squares summed, five exponentials."""
    B, K = source.shape[:2]
    s, t = source.reshape(B, K, -1), target.reshape(B, K, -1)
    n = 2 * B
    total_loss = 0
    for k in range(K):
        x = torch.cat([s[:, k], t[:, k]], 0)
        d = ((x.unsqueeze(0) - x.unsqueeze(1)) ** 2).sum(2)
        bw = d.detach().sum() / (n * n - n) / kernel_mul ** (kernel_num // 2)
        km = sum(torch.exp(-d / (bw * kernel_mul ** m)) for m in range(kernel_num))
        total_loss = total_loss + torch.mean(km[:B, :B] + km[B:, B:] - km[:B, B:] - km[B:, :B])
    return total_loss / K


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def blobs(B, K, S, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    c = torch.rand(2, B, K, 1, 1, generator=gen) * (S - 1)
    yy, xx = torch.arange(S).view(1, 1, S, 1), torch.arange(S).view(1, 1, 1, S)
    g = torch.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / 8.0) + 0.02 * torch.randn(B, K, S, S, generator=gen)
    return g.to(dev).contiguous()


def training(arch, dev, with_mmd):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if with_mmd:
        step.mmd = MMDAlign(weight=0.1)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--block', type=int, default=20)
    ap.add_argument('--skip-iteration', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('bf16')

    # ---- the launches on their own, beside the torch expression
    B, K, S = a.b, 21, a.size // 4
    y_s, y_t = blobs(B, K, S, dev, 1), (0.7 * blobs(B, K, S, dev, 2)).contiguous()
    crit = MMD_loss3()
    for what, req in (('target gradient only (the iteration)', (False, True)), ('both gradients', (True, True))):
        s, t = y_s.clone().requires_grad_(req[0]), y_t.clone().requires_grad_(req[1])
        ms = timed(lambda: crit(s, t), 50)
        print('mmd kernels, %d + %d x %d x %dx%d, %s: %.4f ms per call (distances, coefficients + loss, gradient, sum)' % (B, B, K, S, S, what, ms))
    ops.prof_reset(); ops.prof_enable(2)
    s, t = y_s.clone(), y_t.clone().requires_grad_(True)
    for _ in range(5):
        crit(s, t)
    torch.cuda.synchronize()
    per = {}
    for e in ops.prof_launches():
        per.setdefault(e['label'], []).append(e['us'])
    ops.prof_enable(0); ops.prof_reset()
    for label, us in per.items():
        print('  %-44s %.1f us (event-timed, median of %d)' % (label, statistics.median(us), len(us)))
    s, t = y_s.clone(), y_t.clone().requires_grad_(True)

    def torch_fwd_bwd():
        t.grad = None
        torch_expression(s, t).backward()

    ms_t = timed(torch_fwd_bwd, 3, warm=1)
    got = crit(s, t)
    want = torch_expression(s, t)
    print('torch expression of the reference, forward + backward (target gradient): %.2f ms per call; loss %.6f against %.6f from the kernels'
          % (ms_t, float(want.detach()), float(got.detach())))
    print('peak memory of the torch expression: %.0f MB' % (torch.cuda.max_memory_allocated() / 2 ** 20))
    if a.skip_iteration:
        return

    # ---- the iteration in graph replay, off against on
    del s, t
    torch.cuda.empty_cache()
    batch = make_batch(a.b, a.size, a.size // 4, seed=1, device=dev)
    steps = {k: training(a.arch, dev, k == 'on') for k in ('off', 'on')}
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
        print('mmd %-3s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
    print('difference of the medians: %.3f ms' % (statistics.median(ms['on']) - statistics.median(ms['off'])))
    print('loss_mmd of the last replay: %.6f' % float(steps['on'].out['loss_mmd']))


if __name__ == '__main__':
    main()
