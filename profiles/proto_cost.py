"""Cost of the prototype alignment term: the proto_ launches at B = 64, K = 21, C = 256, 64 x 64, bf16
beside the reference's torch expression for lossx (the Python loop over B x 21 windows with four host reads each, the batch mean,
the blend with the memory, forward and backward through autograd) on the same GPU; then graph replay of the ResNet-50 iteration at
B = 64, 256x256, bf16 with `proto` off against on, alternating blocks of replays of two otherwise identical trainings in one
process.

    python profiles/proto_cost.py [--arch resnet50] [-b 64] [--rounds 6] [--block 20] [--skip-iteration]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

import torch
import torch.nn.functional as F

import mi355
import uda.model as models
from mi355 import ops
from mi355.da_step import PrototypeAlign, build_training
from uda.model.loss import lossx, prototype, prototype_kl_loss
from uda.model.pose_resnet2 import Upsampling
from uda.model.regda_7 import PoseResNetx9
from utils.synthetic import make_batch


def torch_prototype(feature, pre, memory, radius=6, m=0.999):
    """lossx.loss1 as the reference writes it: one slice per (b, j), its bounds read on the host (x selects the rows), each
    window divided by its own s1 * s2; the batch mean; the blend with the memory."""
    B, C, H, W = feature.shape
    rows = []
    for b in range(B):
        per = []
        for j in range(pre.shape[1]):
            x, y = pre[b, j, 0], pre[b, j, 1]
            r0, r1 = int(torch.clamp(x - radius, min=0)), int(torch.clamp(x + radius, max=H - 1))
            q0, q1 = int(torch.clamp(y - radius, min=0)), int(torch.clamp(y + radius, max=W - 1))
            per.append(feature[b, :, r0:r1, q0:q1].sum(dim=(1, 2)) / ((r1 - r0 + 1) * (q1 - q0 + 1)))
        rows.append(torch.stack(per))
    return m * (torch.stack(rows).sum(dim=0) / B) + (1 - m) * memory


def torch_expression(f1, f2, pre1, pre2, mem1, mem2):
    a = F.log_softmax(torch_prototype(f1, pre1, mem1), dim=-1)
    b = torch_prototype(f2, pre2, mem2)
    b = b / b.sum(dim=-1, keepdim=True)
    return F.kl_div(a, b, reduction='none').sum(dim=-1).mean()


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


def training(arch, dev, with_proto):
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=64)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    if with_proto:
        step.proto = PrototypeAlign()
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
    B, K, C, S = a.b, 21, 256, a.size // 4
    gen = torch.Generator().manual_seed(1)
    mk = lambda: torch.relu(torch.randn(B, C, S, S, generator=gen)).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    f_t, f_s = mk(), mk()
    xy_t = (8 + torch.rand(B, K, 2, generator=gen) * (S - 16)).round().to(dev)
    xy_s = (8 + torch.rand(B, K, 2, generator=gen) * (S - 16)).round().to(dev)
    for what, req in (('target gradient only', (True, False)), ('both gradients', (True, True))):
        x, y = f_t.clone().requires_grad_(req[0]), f_s.clone().requires_grad_(req[1])
        crit = lossx()

        def fwd_bwd():
            x.grad = None
            y.grad = None
            crit(x, y, xy_t, xy_s).backward()

        print('proto kernels, B %d K %d C %d %dx%d bf16, %s: %.4f ms per call (two pools, two updates, KL, sum, scatter(s))'
              % (B, K, C, S, S, what, timed(fwd_bwd, 50)))
    # what the iteration adds: the source prototypes exist since step A; pool, update, KL, sum and one scatter
    blend, mem_s, mem_t = ops.proto_blend(0.999, device=dev), torch.zeros(K, C, device=dev), torch.zeros(K, C, device=dev)
    proto_s = prototype(f_s, xy_s, mem_s, blend)
    x = f_t.clone().requires_grad_(True)

    def step_c():
        x.grad = None
        prototype_kl_loss(prototype(x, xy_t, mem_t, blend), proto_s, 'kl').backward()

    print('proto kernels, step C alone (pool, update, KL, sum, scatter): %.4f ms per call' % timed(step_c, 50))
    ops.prof_reset(); ops.prof_enable(2)
    buf = torch.zeros_like(x)
    for _ in range(5):
        step_c()
        gt = ops.proto_kl(prototype(x.detach(), xy_t, mem_t, blend), proto_s, True, False)[1]
        ops.proto_scatter(gt, xy_t, blend, buf, True)
    torch.cuda.synchronize()
    per = {}
    for e in ops.prof_launches():
        per.setdefault(e['label'], []).append((e['us'], e['bytes']))
    ops.prof_enable(0); ops.prof_reset()
    for label, v in per.items():
        us = statistics.median(u for u, _ in v)
        extra = '  %.2f TB/s' % (v[0][1] / us / 1e6) if label.startswith('proto_scatter') else ''
        print('  %-52s %.1f us (event-timed, median of %d)%s' % (label, us, len(v), extra))
    x32, y32 = f_t.float().contiguous().requires_grad_(True), f_s.float().contiguous()
    z = torch.zeros(K, C, device=dev)

    def torch_fwd_bwd():
        x32.grad = None
        torch_expression(x32, y32, xy_t, xy_s, z, z).backward()

    ms_t = timed(torch_fwd_bwd, 2, warm=1)
    got = lossx()(f_t, f_s, xy_t, xy_s)
    want = torch_expression(x32, y32, xy_t, xy_s, z, z)
    print('torch expression of the reference (lossx), forward + backward (target gradient), fp32 NCHW features: %.1f ms per call; loss %.6f against %.6f from the kernels'
          % (ms_t, float(want.detach()), float(got.detach())))
    if a.skip_iteration:
        return

    # ---- the iteration in graph replay, off against on
    del x, x32, y32, buf, f_t, f_s
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
        print('proto %-3s replay: median %.3f ms / iteration  (blocks of %d: %s)' % (k, statistics.median(v), a.block, ' '.join('%.3f' % x for x in v)))
    print('difference of the medians: %.3f ms' % (statistics.median(ms['on']) - statistics.median(ms['off'])))
    print('loss_proto of the last replay: %.6f' % float(steps['on'].out['loss_proto']))


if __name__ == '__main__':
    main()
