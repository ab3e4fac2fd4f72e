"""Flip test and sub-pixel decode (`--flip-test`, `--decode quarter|taylor`; DESIGN.md section 7 "Flip test and sub-pixel decode"):

  1. mi355_flip_decode on 1344 maps of 64 x 64 (B = 64, K = 21) with hm_flip, modes 0 / 1 / 2, against what the parent commit
     could compose for the same average and arg-max: torch.flip + add + scale + ops.argmax2d.  Device events, warm-up first, the
     two forms interleaved (A, B, A, B ...), and a check that both give the same average and indices;
  2. train1.validate() over a synthetic split of 256 images of 256 x 256 (ResNet-50, batch 64) under every --decode with and
     without --flip-test: wall time of a pass after a warm one, images / s, and the EPE / AUC line the pass printed.  Synthetic
     data and a seeded random network: the lines record that the numbers move with the setting, nothing about accuracy.

    python profiles/flip_decode_bench.py [--reps 30] [--out profiles/flip_decode.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from contextlib import redirect_stdout

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import mi355
from mi355 import ops


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out          # microseconds


def kernel_against_composition(reps, dev):
    B, K, S = 64, 21, 64
    g = torch.Generator(device='cpu').manual_seed(5)
    hm, hf = torch.randn(B, K, S, S, generator=g).to(dev), torch.randn(B, K, S, S, generator=g).to(dev)

    def composed():
        avg = (hm + torch.flip(hf, dims=[3])) * 0.5
        return ops.argmax2d(avg) + (avg,)

    out = {'maps': B * K, 'size': S, 'reps': reps, 'bytes_read': 2 * 4 * B * K * S * S}
    for _ in range(3):
        composed()
        for mode in ops.DECODE_MODES:
            ops.flip_decode(hm, hf, 0, mode, want_avg=True)
    torch.cuda.synchronize()
    for mode in ops.DECODE_MODES:
        for shift, want_avg in ((0, True), (1, True), (1, False)):
            fused = lambda: ops.flip_decode(hm, hf, shift, mode, 2.0, (4., 4.), want_avg=want_avg)
            tf, tc = [], []
            for _ in range(reps):
                t, f = timed(fused); tf.append(t)
                t, c = timed(composed); tc.append(t)
            same = None
            if shift == 0:
                same = bool(torch.equal(f[0], c[0])) and bool(torch.equal(f[3], c[3])) and bool(torch.equal(f[2], c[2]))
            key = 'mode_%s_shift%d%s' % (mode, shift, '' if want_avg else '_no_avg')
            out[key] = {'fused_us_median': statistics.median(tf), 'fused_us_min': min(tf), 'fused_us_max': max(tf),
                        'composed_us_median': statistics.median(tc), 'composed_us_min': min(tc), 'composed_us_max': max(tc),
                        'composed_over_fused': statistics.median(tc) / statistics.median(tf), 'same_avg_idx_maxval': same}
            print(key, json.dumps(out[key]))
    return out


def validate_settings(dev, passes):
    import train1
    import uda.model as models
    from seeded import fill_module_
    from torch.utils.data import DataLoader
    from uda.model.loss import JointsKLLoss
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic_dataset import SyntheticHand21
    bb = models.resnet50(pretrained=False)
    m = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True)
    fill_module_(m, 11)
    m = m.to(dev)
    n_img = 256
    loader = DataLoader(SyntheticHand21(n_img, (256, 256), (64, 64), seed=14), batch_size=64)
    batches = [b for b in loader]                 # the data set's CPU work is not what is compared

    class Held:
        dataset = loader.dataset

        def __iter__(self):
            return iter(batches)

        def __len__(self):
            return len(batches)

    out = {'images': n_img, 'arch': 'resnet50', 'image_size': 256, 'batch': 64, 'passes_timed': passes}
    for decode in ('argmax', 'upsample', 'quarter', 'taylor'):
        for flip in (False, True):
            args = argparse.Namespace(print_freq=100, metrics='full', decode=decode, auc_max_px=30.0, flip_test=flip, flip_shift=1, decode_sigma=None)
            ts, text = [], ''
            for i in range(passes + 1):
                torch.cuda.synchronize()
                buf = io.StringIO()
                t0 = time.time()
                with redirect_stdout(buf):
                    train1.validate(Held(), m, JointsKLLoss(), args)
                torch.cuda.synchronize()
                ts.append((time.time() - t0) * 1e3)
                text = buf.getvalue()
            line = [l for l in text.splitlines() if l.startswith('EPE: ')][0]
            med = statistics.median(ts[1:])
            key = '%s%s' % (decode, '_flip' if flip else '')
            out[key] = {'ms_per_pass_median': med, 'ms_passes': ts[1:], 'images_per_s': n_img / med * 1e3, 'line': line}
            print(key, json.dumps(out[key]))
    for decode in ('argmax', 'upsample', 'quarter', 'taylor'):
        out[decode + '_flip']['time_over_no_flip'] = out[decode + '_flip']['ms_per_pass_median'] / out[decode]['ms_per_pass_median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(HERE, 'flip_decode.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('flip_decode_bench needs the GPU: nothing here is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    res = {'device': torch.cuda.get_device_name(0), 'kernel': kernel_against_composition(a.reps, dev), 'validate': validate_settings(dev, a.passes)}
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    bad = [k for k, v in res['kernel'].items() if isinstance(v, dict) and v['same_avg_idx_maxval'] is False]
    if bad:
        raise SystemExit('flip_decode and the composition disagree: %s' % bad)


if __name__ == '__main__':
    main()
