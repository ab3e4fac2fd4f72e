"""Image-resolution decode: the fused mi355_upsample_argmax against the pair it replaces (ops.bilinear_up, which writes the
up-sampled maps, then ops.argmax2d, which reads them back), and the wall time of one train1.validate() pass per --metrics /
--decode setting.  One process, device events, warm-up first, the two forms interleaved (A, B, A, B ...).

    python profiles/decode_bench.py [--reps 20] [--no-validate] > profiles/decode_bench.txt

Per shape: median and min / max of the per-repetition times of both forms, the factor pair / fused, the bytes the algorithm
needs (fused: the input maps; pair: input + up-sampled maps written and read) over the median times, and a check that both
forms return the same indices."""
import argparse
import os
import statistics
import sys
import time

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


def decode(rows, h, H, reps, dev):
    hm = torch.randn(rows // 21, 21, h, h, device=dev)
    up = torch.empty((rows // 21, 21, H, H), dtype=torch.float32, device=dev)
    out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in (((rows // 21, 21), torch.int32), ((rows // 21, 21, 2), torch.float32),
                                                                   ((rows // 21, 21, 1), torch.float32)))
    fused = lambda: ops.upsample_argmax(hm, H, out=out)

    def pair():
        mi355.call('mi355_bilinear_up', hm.data_ptr(), up.data_ptr(), rows, h, h, H, H, 1.0, 0, mi355.stream_ptr())
        return ops.argmax2d(up)

    for _ in range(3):
        fused(); pair()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(reps):
        t, f = timed(fused); tf.append(t)
        t, p = timed(pair); tp.append(t)
    same = bool(torch.equal(f[0], p[0])) and bool(torch.equal(f[1], p[1]))
    mf, mp = statistics.median(tf), statistics.median(tp)
    in_b, up_b = 4.0 * rows * h * h, 4.0 * rows * H * H
    print('rows %d  %dx%d -> %dx%d  (%d repetitions, interleaved)' % (rows, h, h, H, H, reps))
    print('  fused upsample_argmax : median %8.1f us  (min %8.1f, max %8.1f)  %6.1f GB/s of %5.1f MB' % (mf, min(tf), max(tf), in_b / mf / 1e3, in_b / 1e6))
    print('  bilinear_up + argmax2d: median %8.1f us  (min %8.1f, max %8.1f)  %6.1f GB/s of %5.1f MB' % (mp, min(tp), max(tp), (in_b + 2 * up_b) / mp / 1e3, (in_b + 2 * up_b) / 1e6))
    print('  pair / fused = %.2f   same idx and xy: %s' % (mp / mf, same))
    return mp / mf, same


def validate_times(dev):
    import train1
    import uda.model as models
    from seeded import fill_module_
    from torch.utils.data import DataLoader
    from uda.model.loss import JointsKLLoss
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic_dataset import SyntheticHand21
    bb = models.resnet18(pretrained=False)
    m = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True)
    fill_module_(m, 11)
    m = m.to(dev)
    loader = DataLoader(SyntheticHand21(4 * 64, (256, 256), (64, 64), seed=14), batch_size=64)
    batches = [b for b in loader]                 # the data set's CPU work is not what is compared

    class Held:
        dataset = loader.dataset

        def __iter__(self):
            return iter(batches)

        def __len__(self):
            return len(batches)

    print('one validate() pass, synthetic test split (256 images of 256 x 256, resnet18, batch 64), wall time after a warm pass:')
    devnull = open(os.devnull, 'w')
    for name, kw in (('--metrics pck', {}), ('--metrics full', dict(metrics='full', decode='argmax', auc_max_px=30.0)),
                     ('--metrics full --decode upsample', dict(metrics='full', decode='upsample', auc_max_px=30.0))):
        args = argparse.Namespace(print_freq=100, **kw)
        ts = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.time()
            old, sys.stdout = sys.stdout, devnull
            try:
                train1.validate(Held(), m, JointsKLLoss(), args)
            finally:
                sys.stdout = old
            torch.cuda.synchronize()
            ts.append((time.time() - t0) * 1e3)
        print('  %-34s %7.1f ms  (passes after the first: %s)' % (name, statistics.median(ts[1:]), ' '.join('%.1f' % t for t in ts[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-validate', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('decode_bench needs the GPU: nothing here is measured without one')
    dev = torch.device('cuda:0')
    mi355.load()
    print('device: %s' % torch.cuda.get_device_name(0))
    ok = True
    for rows, h, H in ((1344, 64, 256), (672, 128, 512)):
        ratio, same = decode(rows, h, H, a.reps, dev)
        ok = ok and same
    if not a.no_validate:
        validate_times(dev)
    if not ok:
        raise SystemExit('the fused decode and the pair disagree')


if __name__ == '__main__':
    main()
