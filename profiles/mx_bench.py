"""'mxfp8' compute mode measured against 'bf16' and 'fp8' (run on an MI355X from the repository root):

    python profiles/mx_bench.py layers      > profiles/mx_layers.txt        # (a) per-layer GEMM times + the MX quantiser
    python profiles/mx_bench.py converge    > profiles/mx_convergence.txt   # (b) convergence table + (c) ms per replayed iteration
    python profiles/mx_bench.py eval        >> profiles/mx_eval.txt         # (d) the inference launches of the MX-eval switch

(a) Operands from HBM, 20 warm-up + 50 timed launches per layer between two events (ResNet-50 256x256, B=64 shapes).  Kernel-only
    durations: run the same command under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/mx_bench.py layers`.
(b) The construction of bench.py (ResNet-50, 256x256, B=64, seed 1, the fixed synthetic batch, 3 eager iterations, capture, then
    replay): loss_s after `bench.py --steps 600 --warmup 5` (605 iterations) and after --steps 900 -- for bf16, fp8,
    fp8 + MI355_FP8_DECONV=1 and mxfp8, each mode in a fresh child process (the fp8 switches are read at import).  The bf16 row is
    first checked against `bench.py --dtype bf16 --steps 600 --warmup 5`'s losses_last_step, bit for bit.
(c) ms per replayed iteration: the mean over the last 200 iterations of each run of (b).
(d) The eval-mode (BatchNorm-folded, bias + ReLU in the epilogue) launch of the five neck / head layers and of one backbone 3x3
    conv per stage (ResNet-50 256x256, B=64), timed as (a) times its layers, in three forms: the bf16 folded launch; MX with a
    stand-alone quantise of the input (mx_quantize + mi355_conv_*_mx_act); MX fed by a fused copy (the launch alone, writing the
    MX copy of its own output where its consumer is an MX layer -- which is what a layer behind an MX producer costs).
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd')
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)


def _timeit(fn, warm=20, n=50):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us


def layers():
    import torch
    import mi355
    from mi355 import ops
    mi355.load()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    print('%-44s %10s %10s %10s %10s %9s' % ('layer (B=64)', 'bf16 us', 'fp8 us', 'fp8 plain', 'mx us', 'mx/plain'))
    rows = [  # name, N, H, W, Ci, Co, k, s, p, which: 'fwd' | 'dgrad' | 'deconv'
        ('3x3 256->256 @64x64 forward', 64, 64, 64, 256, 256, 3, 1, 1, 'fwd'),
        ('3x3 256->256 @64x64 input gradient', 64, 64, 64, 256, 256, 3, 1, 1, 'dgrad'),
        ('3x3 s2 256->256 @64x64 forward', 64, 64, 64, 256, 256, 3, 2, 1, 'fwd'),
        ('4x4 s2 transposed 256->256 @32x32->64x64', 64, 64, 64, 256, 256, 4, 2, 1, 'deconv'),
        ('3x3 256->256 @16x16 forward', 64, 16, 16, 256, 256, 3, 1, 1, 'fwd')]
    for name, N, H, W, Ci, Co, k, s, p, which in rows:
        d16 = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, torch.bfloat16)
        d8 = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
        x = torch.randn(N, H, W, Ci, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
        dy = torch.randn(N, d16.Ho, d16.Wo, Co, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
        w = (torch.randn(Co, k * k, Ci, device=dev, generator=g) / (Ci * k * k) ** 0.5).contiguous()
        wf, wt = ops.pack_weights(w, Co, k * k, Ci, Ci, torch.bfloat16)
        st8 = ops.fp8_state(dev)
        wf8, wt8 = ops.pack_weights_fp8(w, Co, k * k, Ci, st8)
        wfm, sfm, wtm, stm = ops.pack_weights_mx(w, Co, k * k, Ci)
        sx, sd = ops.fp8_state(dev), ops.fp8_state(dev)
        x8, dy8 = ops.fp8_quantize(x, sx, ops.E4M3, jit=True), ops.fp8_quantize(dy, sd, ops.E5M2, jit=True)
        dy8e = ops.fp8_quantize(dy, ops.fp8_state(dev), ops.E4M3, jit=True)
        xm, sxm = ops.mx_quantize(x)
        dym, sdym = ops.mx_quantize(dy)
        if which == 'fwd':
            f16, f8, fmx = (lambda: ops.conv_fwd(d16, x, wf)), (lambda: ops.conv_fwd_fp8(d8, x8, sx, wf8, st8)), \
                (lambda: ops.conv_fwd_mx(d8, xm, sxm, wfm, sfm))
        elif which == 'dgrad':
            f16, f8, fmx = (lambda: ops.conv_dgrad(d16, dy, wt)), (lambda: ops.conv_dgrad_fp8(d8, dy8, sd, wt8, st8)), \
                (lambda: ops.conv_dgrad_mx(d8, dym, sdym, wtm, stm))
        else:      # transposed conv forward = conv-form input gradient with the deconv input (e4m3 in both fp8 forms) gathered
            f16, f8, fmx = (lambda: ops.conv_dgrad(d16, dy, wt)), (lambda: ops.conv_dgrad_fp8(d8, dy8e, sd, wt8, st8, dy_fmt=ops.E4M3)), \
                (lambda: ops.conv_dgrad_mx(d8, dym, sdym, wtm, stm))
        t = [_timeit(f16), _timeit(f8)]
        prev = mi355.load().mi355_set_fp8_kw3(0)       # the fp8 kernel without its row-sharing variant (MX has none)
        t.append(_timeit(f8))
        mi355.load().mi355_set_fp8_kw3(prev)
        t.append(_timeit(fmx))
        print('%-44s %10.1f %10.1f %10.1f %10.1f %9.3f' % (name, t[0], t[1], t[2], t[3], t[3] / t[2]))
    x = torch.randn(64, 64, 64, 256, device=dev, generator=g).to(torch.bfloat16)          # the 134-MB activation
    q, sc = ops.mx_quantize(x)
    tq = _timeit(lambda: ops.mx_quantize(x, q, sc))
    st = ops.fp8_state(dev)
    ops.fp8_quantize(x, st, ops.E4M3, jit=True)
    t8 = _timeit(lambda: ops.fp8_quantize(x, st, ops.E4M3))
    n = x.numel()
    print('\nmx_quantize bf16 [262144][256] (134 MB): %.1f us, %.2f TB/s (2 B read + 1 + 1/32 B written per element)'
          % (tq, n * (2 + 1 + 1 / 32) / tq / 1e6))
    print('fp8_quantize (per-tensor, delayed) same tensor: %.1f us, %.2f TB/s' % (t8, n * 3 / t8 / 1e6))


def eval_layers():
    import torch
    import mi355
    from mi355 import ops
    mi355.load()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    print('%-46s %10s %12s %12s %10s %10s' % ('layer (B=64, eval: + bias + ReLU)', 'bf16 us', 'mx+quant us', 'mx fused us', 'quant us', 'fused/bf16'))
    rows = [  # name, N, conv-form H, W, Ci, Co, k, s, p, kind, writes the copy for its consumer
        ('4x4 s2 transposed 2048->256 @8x8->16x16', 64, 16, 16, 256, 2048, 4, 2, 1, 'deconv', True),
        ('4x4 s2 transposed 256->256 @16x16->32x32', 64, 32, 32, 256, 256, 4, 2, 1, 'deconv', True),
        ('4x4 s2 transposed 256->256 @32x32->64x64', 64, 64, 64, 256, 256, 4, 2, 1, 'deconv', True),
        ('3x3 256->256 @64x64 (head, first)', 64, 64, 64, 256, 256, 3, 1, 1, 'conv', True),
        ('3x3 256->256 @64x64 (head, last 3x3)', 64, 64, 64, 256, 256, 3, 1, 1, 'conv', False),
        ('3x3 128->128 @32x32 (layer2 conv2)', 64, 32, 32, 128, 128, 3, 1, 1, 'conv', False),
        ('3x3 256->256 @16x16 (layer3 conv2)', 64, 16, 16, 256, 256, 3, 1, 1, 'conv', False),
        ('3x3 512->512 @8x8 (layer4 conv2)', 64, 8, 8, 512, 512, 3, 1, 1, 'conv', False)]
    for name, N, H, W, Ci, Co, k, s, p, kind, copy in rows:
        d16 = ops.make_desc(N, H, W, Ci, Co, k, k, s, p, torch.bfloat16)
        d8 = ops.make_desc_fp8(N, H, W, Ci, Co, k, k, s, p)
        w = (torch.randn(Co, k * k, Ci, device=dev, generator=g) / (Ci * k * k) ** 0.5).contiguous()
        wf, wt = ops.pack_weights(w, Co, k * k, Ci, Ci, torch.bfloat16)
        wfm, sfm, wtm, stm = ops.pack_weights_mx(w, Co, k * k, Ci)
        if kind == 'conv':
            x = torch.randn(N, H, W, Ci, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
            bias = torch.randn(Co, device=dev, generator=g)
            y = ops.nhwc_empty(N, Co, d16.Ho, d16.Wo, torch.bfloat16, dev)
            f16 = lambda: ops.conv_fwd(d16, x, wf, bias, None, relu=True)
            fmx = lambda: ops.conv_fwd_mx_act(d8, xm, sxm, wfm, sfm, bias, relu=True, out=y, out8=y8, out_scales=sy)
        else:       # the deconv input is the conv-form's output side
            x = torch.randn(N, d16.Ho, d16.Wo, Co, device=dev, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
            bias = torch.randn(Ci, device=dev, generator=g)
            y = ops.nhwc_empty(N, Ci, H, W, torch.bfloat16, dev)
            f16 = lambda: ops.deconv_fwd_act(d16, x, wt, bias, relu=True)
            fmx = lambda: ops.conv_dgrad_mx_act(d8, xm, sxm, wtm, stm, bias, relu=True, out=y, out8=y8, out_scales=sy)
        xm, sxm = ops.mx_quantize(x)
        y8 = torch.empty_strided(y.shape, y.stride(), dtype=torch.uint8, device=dev) if copy else None
        sy = torch.empty(y.numel() // 32, dtype=torch.uint8, device=dev) if copy else None
        tq = _timeit(lambda: ops.mx_quantize(x, xm, sxm))
        t16, tmx = _timeit(f16), _timeit(fmx)
        tboth = _timeit(lambda: (ops.mx_quantize(x, xm, sxm), fmx()))
        print('%-46s %10.1f %12.1f %12.1f %10.1f %10.3f' % (name + (' +copy' if copy else ''), t16, tboth, tmx, tq, tmx / t16))


def converge_child(mode, iters_list):
    """one mode, bench.py's construction; prints a JSON line"""
    import torch
    import mi355
    from mi355.da_step import build_training
    import uda.model as models
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic import make_batch
    dev = torch.device('cuda:0')
    mi355.load()
    mi355.set_compute_dtype('fp8' if mode.startswith('fp8') else mode)
    torch.manual_seed(1)
    S, B = 256, 64
    backbone = models.__dict__['resnet50'](pretrained=False)
    model = PoseResNetx9(backbone, Upsampling(backbone.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=S // 4)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    batch = make_batch(B, S, S // 4, seed=1, device=dev)
    out, rec, t0 = None, {}, None
    total = max(iters_list) + 5
    for it in range(total):
        if it == 3:
            step.capture(batch, warmup=0)
        if it == total - 200:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        out = step.run(batch)
        for s in scheds.values():
            s.step()
        if it + 1 - 5 in iters_list:                 # (reading the losses synchronises: only at the recorded iterations)
            rec[it + 1 - 5] = [float(out[k]) for k in ('loss_s', 'loss_gf', 'loss_gt')]
    torch.cuda.synchronize()
    print(json.dumps({'mode': mode, 'losses': rec, 'ms_per_iteration': 1e3 * (time.perf_counter() - t0) / 200}))


def converge():
    env0 = {k: v for k, v in os.environ.items() if not k.startswith('MI355_FP8_')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '600', '--warmup', '5',
                        '--dtype', 'bf16'], env=env0, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
    bench_losses = json.loads(line)['losses_last_step']
    res = {}
    for mode, extra in (('bf16', {}), ('fp8', {}), ('fp8+deconv', {'MI355_FP8_DECONV': '1'}), ('mxfp8', {})):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'converge-child', mode], env=dict(env0, **extra),
                           capture_output=True, text=True, timeout=1800, cwd=ROOT)
        if r.returncode:
            raise SystemExit(r.stdout[-2000:] + r.stderr[-3000:])
        res[mode] = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        print(json.dumps(res[mode]), flush=True)
    mine = res['bf16']['losses']['600']
    bench_losses = [bench_losses[k] for k in ('loss_s', 'loss_gf', 'loss_gt')]
    same = [float(a) for a in mine] == [float(b) for b in bench_losses]
    print('bench.py --dtype bf16 --steps 600 --warmup 5 losses_last_step: %s' % (bench_losses,))
    print('this script, bf16, after 600:                          %s  -> %s' % (mine, 'bit-identical' if same else 'DIFFERENT'))
    print('\nResNet-50 256x256 B=64, fixed synthetic batch: supervised loss_s after 600 [900] iterations; ms per replayed iteration')
    for mode, v in res.items():
        print('  %-12s %8.3f [%8.3f]   %.2f ms' % (mode, v['losses']['600'][0], v['losses']['900'][0], v['ms_per_iteration']))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'layers'
    if what == 'layers':
        layers()
    elif what == 'eval':
        eval_layers()
    elif what == 'converge':
        converge()
    elif what == 'converge-child':
        converge_child(sys.argv[2], [600, 900])
    else:
        raise SystemExit(__doc__)
