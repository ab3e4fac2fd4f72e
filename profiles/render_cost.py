"""Cost of the rendered hand data path (DESIGN.md section 7 "Rendered hands"): `mi355_render_hands` at B = 64, 256 x 256 with and
without `out_ema`, on 'cg' and on 'photo' records, beside `mi355_affine_warp_images` on an output of the same size and the two
launches of `mi355.augment.augment` (with image_ema) on 64 ragged sources, each between device events in alternating rounds; the
histogram of primitives that survive the per-tile culling (the kernel's rule, restated on the host); the loader's throughput in
records / s at -j 0 and -j 4; and the time of a training iteration fed by `--synthetic-hands` against one fed by `--synthetic`,
alternating blocks of graph replays of one training in one process.  Prints one line per figure and, last, one JSON line with all.

    python profiles/render_cost.py [--arch resnet50] [-b 64] [--rounds 5] [--block 20] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

import numpy as np
import torch

import mi355
from mi355 import ops
from utils.data import DevicePrefetcher, ForeverDataIterator, RenderedHandIterator, record_collate
from utils.rendered_dataset import RenderedHand21


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


def records(domain, n, S, seed=3):
    ds = RenderedHand21(length=n, image_size=S, heatmap_size=S // 4, seed=seed, domain=domain)
    return np.array([ds[i][0] for i in range(n)])


def kernel_constant(name):
    """A constexpr of csrc/render.hip, so that the host restatement below cannot drift from the kernel unnoticed."""
    import re
    src = open(os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd', 'csrc', 'render.hip')).read()
    return float(re.search(r'constexpr \w+ %s = ([0-9.]+)f?;' % name, src).group(1))


def primitives(rec, max_coord=1048576.0):
    """(ax, ay, bx, by, r) of the valid primitives of one record (include/mi355pose.h: every magnitude <= 2^20, r > 0)."""
    out = []
    for k in range(21):
        if k < 20:
            ja, jb = (0 if k % 4 == 0 else k), k + 1
            v = (rec['jx'][ja], rec['jy'][ja], rec['jz'][ja], rec['jx'][jb], rec['jy'][jb], rec['jz'][jb], rec['radius'][k])
        else:
            v = (rec['occ_a'][0], rec['occ_a'][1], rec['occ_z'], rec['occ_b'][0], rec['occ_b'][1], rec['occ_z'], rec['occ_r'])
        if all(abs(float(x)) <= max_coord for x in v) and float(v[6]) > 0:
            out.append((float(v[0]), float(v[1]), float(v[3]), float(v[4]), float(v[6])))
    return out


def tile_histogram(recs, S):
    """Primitives kept per (sample, tile) by the kernel's culling rule (csrc/render.hip: bounding box of the capsule against the
    tile's sample points, RH_CULL_MARGIN pixels of margin; tile and margin are read from the kernel's source), as counts[k] = tiles
    that keep k primitives, k = 0 .. 21."""
    tile, margin = int(kernel_constant('RH_TILE')), kernel_constant('RH_CULL_MARGIN')
    counts = np.zeros(22, dtype=np.int64)
    for rec in recs:
        prims = primitives(rec)
        for ty in range(0, S, tile):
            for tx in range(0, S, tile):
                xlo, xhi, ylo, yhi = tx - 0.25 - margin, tx + tile - 1 + 0.25 + margin, ty - 0.25 - margin, ty + tile - 1 + 0.25 + margin
                k = sum(1 for ax, ay, bx, by, r in prims
                        if min(ax, bx) - r <= xhi and max(ax, bx) + r >= xlo and min(ay, by) - r <= yhi and max(ay, by) + r >= ylo)
                counts[k] += 1
    return counts.tolist()


def augment_batch(B):
    import uda.dataset.keypoint_detection as T
    from PIL import Image
    from utils.data import ragged_collate
    rng = np.random.default_rng(1)
    items = []
    for _ in range(B):
        side = int(rng.integers(200, 480))
        im = Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8))
        s, e = T.DeviceAugment(180, 256)(im, keypoint2d=rng.uniform(0, side, (21, 2)), intrinsic_matrix=np.eye(3))
        items.append((s, torch.from_numpy(e['keypoint2d']), torch.ones(21, 1), {}))
    packed, table, params, _, _, _ = ragged_collate(items)
    return packed.cuda(), table, params


def kernel_figures(dev, B, S, reps, rounds):
    from mi355.augment import augment
    host = {d: records(d, B, S) for d in ('cg', 'photo')}
    recs = {d: torch.from_numpy(h.view(np.uint8).reshape(B, -1).copy()).to(dev) for d, h in host.items()}
    out, ema = torch.empty(B, 3, S, S, device=dev), torch.empty(B, 3, S, S, device=dev)
    x = torch.randn(B, 3, S, S, device=dev)
    view = torch.from_numpy(ops.view_records(np.linspace(-30, 30, B), np.linspace(0.8, 1.2, B), np.zeros((B, 2)), S, S // 4)).to(dev)
    calls = {
        'render_photo': lambda: ops.render_hands(recs['photo'], S, out=out),
        'render_photo_ema': lambda: ops.render_hands(recs['photo'], S, out=out, out_ema=ema),
        'render_cg': lambda: ops.render_hands(recs['cg'], S, out=out),
        'render_cg_ema': lambda: ops.render_hands(recs['cg'], S, out=out, out_ema=ema),
        'affine_warp_images': lambda: ops.affine_warp_images(x, view, out=out),
    }
    if S == 256:
        packed, table, params = augment_batch(B)
        calls['augment_pair_with_ema'] = lambda: augment(packed, table, params, want_ema=True)
    ms = {k: [] for k in calls}
    for _ in range(rounds):                                   # alternating, so that clocks and neighbours hit all alike
        for k, fn in calls.items():
            ms[k].append(timed(fn, reps, warm=3))
    res = {'B': B, 'image': S, 'reps': reps, 'calls': {}}
    nout = 4.0 * B * 3 * S * S
    for k, v in ms.items():
        med = statistics.median(v)
        nbytes = nout * (2 if k.endswith('_ema') else 1) if k.startswith('render') else None
        res['calls'][k] = {'us': med * 1e3, 'us_rounds': [t * 1e3 for t in v], 'store_bytes': nbytes,
                           'store_TBps': nbytes / med / 1e9 if nbytes else None}
        print('%-24s %8.1f us (rounds %s)%s' % (k, med * 1e3, ' '.join('%.1f' % (t * 1e3) for t in v),
                                               ', stores %.1f MB -> %.2f TB/s' % (nbytes / 1e6, nbytes / med / 1e9) if nbytes else ''))
    for d in host:
        h = tile_histogram(host[d], S)
        tiles = sum(h)
        res['tile_histogram_' + d] = h
        res['tile_mean_kept_' + d] = sum(k * c for k, c in enumerate(h)) / tiles
        print('%s: %d tiles, kept primitives per tile: mean %.2f, empty %.0f %%, histogram %s' % (d, tiles, res['tile_mean_kept_' + d],
                                                                                               100.0 * h[0] / tiles, h))
    return res


def loader_rate(ds, workers, collate, batch=64, batches=40):
    from torch.utils.data import DataLoader
    ld = DataLoader(ds, batch_size=batch, shuffle=True, num_workers=workers, collate_fn=collate, drop_last=True,
                    persistent_workers=workers > 0)
    it = iter(ld)
    for _ in range(max(2 * workers, 1)):                      # worker start-up and the first round of prefetched batches
        next(it)
    t0 = time.perf_counter()
    for _ in range(batches):
        next(it)
    return batches * batch / (time.perf_counter() - t0)


def loader_figures(S):
    torch.set_num_threads(1)
    ds = RenderedHand21(length=65536, image_size=S, heatmap_size=S // 4, seed=21, domain='photo')
    res = {'affinity': len(os.sched_getaffinity(0))}
    for j in (0, 4):
        res['records_per_s_j%d' % j] = round(loader_rate(ds, j, record_collate), 1)
        print('loader -j %d: %.0f records / s' % (j, res['records_per_s_j%d' % j]))
    return res


def iteration_figures(dev, arch, B, S, rounds, block, workers):
    """One training, its graphs captured once; blocks of iterations whose batches come from the --synthetic pipeline (noise images
    through DevicePrefetcher) and from the --synthetic-hands pipeline (records through RenderedHandIterator), alternating."""
    import uda.model as models
    from torch.utils.data import DataLoader
    from mi355.da_step import build_training
    from uda.model.pose_resnet2 import Upsampling
    from uda.model.regda_7 import PoseResNetx9
    from utils.synthetic_dataset import SyntheticHand21
    torch.manual_seed(1)
    bb = models.__dict__[arch](pretrained=False)
    model = PoseResNetx9(bb, Upsampling(bb.out_features), 256, 21, num_head_layers=2, finetune=True).to(dev)
    step, opts, scheds = build_training(model, heatmap_size=S // 4)
    for c in step.crit.values():
        if hasattr(c, 'guard_empty_maps'):
            c.guard_empty_maps = True
    n = B * block * (rounds + 2)

    def ld(ds, collate=None):
        return ForeverDataIterator(DataLoader(ds, batch_size=B, shuffle=True, num_workers=workers, pin_memory=True, drop_last=True,
                                              collate_fn=collate, persistent_workers=workers > 0))
    noise = [DevicePrefetcher(ld(SyntheticHand21(n, (S, S), (S // 4, S // 4), seed=s)), dev) for s in (11, 13)]
    hands = [RenderedHandIterator(ld(RenderedHand21(n, S, S // 4, seed=s, domain=d), record_collate), dev, S, S // 4)
             for s, d in ((21, 'cg'), (23, 'photo'))]

    def batch_of(pair):
        (x_s, l_s, w_s, _), (x_t, l_t, w_t, _) = next(pair[0]), next(pair[1])
        return dict(x_s=x_s, label_s=l_s, w_s=w_s, x_t=x_t, w_t=w_t, label_t=l_t)

    first = batch_of(hands)
    for _ in range(3):
        step.run(first)
    step.capture(first, warmup=0)
    ms = {'synthetic': [], 'synthetic_hands': []}
    for r in range(rounds + 1):                               # (the first round warms the loaders' workers and is dropped)
        for name, pair in (('synthetic', noise), ('synthetic_hands', hands)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                step.run(batch_of(pair))
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) / block * 1e3)
    res = {'arch': arch, 'B': B, 'image': S, 'block': block, 'workers': workers}
    for k, v in ms.items():
        res[k + '_ms'], res[k + '_ms_blocks'] = statistics.median(v), v
        print('%-16s median %.2f ms / iteration, %.0f images / s per domain (blocks of %d: %s)' % (
            k, statistics.median(v), B / statistics.median(v) * 1e3, block, ' '.join('%.2f' % t for t in v)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='resnet50')
    ap.add_argument('-b', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--block', type=int, default=20)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('-j', type=int, default=2, help='loader workers per data set of the iteration comparison (four data sets)')
    ap.add_argument('--skip-iteration', action='store_true', help='the launches and the loader only')
    ap.add_argument('--json', default=None, help='also write the result line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    res = {'loader': loader_figures(a.size)}                  # (first: its workers are gone before the GPU is opened)
    mi355.load()
    mi355.set_compute_dtype('bf16')
    res['kernel'] = kernel_figures(dev, a.b, a.size, a.reps, a.rounds)
    if not a.skip_iteration:
        res['iteration'] = iteration_figures(dev, a.arch, a.b, a.size, 3, a.block, a.j)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
