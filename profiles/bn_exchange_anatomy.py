"""Where the time of one bn_bwd_resident_kernel launch goes, by in-kernel stamps.

Needs a library built with the stamps compiled in (they are off in the default build):

    python domain-adaptative-hand-pose-estimation_amd/build.py --variant stamp --flags "-DBN_RES_STAMPS"
    MI355_LIB=scratch/ab/libstamp.so python profiles/bn_exchange_anatomy.py [--reps 7] [--label child]

Thread 0 of every block stores the 100 MHz wall clock at six points: 0 kernel entry, 1 last pass-1 load consumed, 2 partial
sums published, 3 exchange complete (group totals in LDS), 4 first pass-2 store, 5 exit.  Every launch runs behind a 512 MiB
fill that evicts the caches, as a layer's backward finds them in the training step.  Printed per geometry, in microseconds:
the median and the maximum over all blocks of all repetitions of each phase, the spread of stamp 2 over the blocks of a launch
(the exchange cannot end before the last block has published), and the time from that last publish to each block's stamp 3 --
what the exchange itself costs once everybody is there.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'domain-adaptative-hand-pose-estimation_amd'))

# the benchmark's one-launch backward geometries: rows, C, mask mode (2: recomputed from x, 3: bit mask of the forward)
GEOMS = [(262144, 256, 2), (262144, 256, 3), (65536, 512, 3), (16384, 256, 2), (16384, 1024, 3), (65536, 256, 2), (262144, 64, 2),
         (65536, 128, 2), (4096, 2048, 3), (1048576, 64, 2), (4096, 512, 2), (262144, 128, 2), (16384, 512, 2)]
PHASES = [('pass 1', 0, 1), ('fold+publish', 1, 2), ('exchange', 2, 3), ('to 1st store', 3, 4), ('pass 2', 4, 5), ('kernel', 0, 5)]


def blocks_of(rows, C, group_channels=64, ncu=256):
    """The launch plan of bn_resident_plan (csrc/bn.hip): G channel groups x R row blocks."""
    G = C // group_channels
    R = min(ncu // G, rows)
    rpb = -(-rows // R)
    return G, -(-rows // rpb)


def make_case(rows, C, mode, dtype, dev, seed):
    from mi355 import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    N, H, W = (rows // 4096, 64, 64) if rows >= 4096 else (1, 1, rows)
    x, dy = ops.nhwc_empty(N, C, H, W, dtype, dev), ops.nhwc_empty(N, C, H, W, dtype, dev)
    x.permute(0, 2, 3, 1).copy_(torch.randn(N, H, W, C, generator=g, device=dev))
    dy.permute(0, 2, 3, 1).copy_(torch.randn(N, H, W, C, generator=g, device=dev))
    ch = 8 if dtype == torch.bfloat16 else 4
    case = dict(x=x, dy=dy, gamma=1 + 0.1 * torch.randn(C, generator=g, device=dev), beta=0.1 * torch.randn(C, generator=g, device=dev),
                mean=0.1 * torch.randn(C, generator=g, device=dev), invstd=1 + 0.1 * torch.rand(C, generator=g, device=dev), mask=None, mode=mode)
    if mode == 3:
        case['mask'] = torch.randint(0, 256, (rows * C // ch,), generator=g, device=dev, dtype=torch.uint8)
    return case


def run_case(case, want_dres):
    from mi355 import ops
    C = case['x'].shape[1]
    dg, db = torch.zeros(C, device=case['x'].device), torch.zeros(C, device=case['x'].device)
    dx, dres = ops.bn_bwd(case['dy'], case['x'], None, case['gamma'], case['mean'], case['invstd'], dg, db, False, True, want_dres,
                          beta=case['beta'], relu_mask=case['mask'])
    return dx, dres, dg, db


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--label', default=os.path.basename(os.environ.get('MI355_LIB', 'default library')))
    a = ap.parse_args()
    import mi355
    from mi355 import ops
    lib = mi355.load()
    if not hasattr(lib, 'mi355_bn_resident_stamps'):
        sys.exit('this library has no stamps: build it with --flags "-DBN_RES_STAMPS" and point MI355_LIB at it')
    lib.mi355_bn_resident_stamps.restype, lib.mi355_bn_resident_stamps.argtypes = ctypes.c_int, [ctypes.c_void_p]
    lib.mi355_bn_set_resident(1)
    dev = torch.device('cuda:0')
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    buf = np.zeros((256, 8), dtype=np.uint64)
    print('== %s: bn_bwd_resident_kernel by in-kernel stamps, us; median / max over blocks x %d launches behind a cache-evicting fill' % (a.label, a.reps))
    print('%-22s %5s | %s | %13s | %13s' % ('geometry', 'grid', ' | '.join('%13s' % n for n, _, _ in PHASES), 'publish skew', 'last pub -> 3'))
    for rows, C, mode in GEOMS:
        case = make_case(rows, C, mode, torch.bfloat16, dev, 1)
        G, R = blocks_of(rows, C)
        n = G * R
        run_case(case, mode == 3)
        torch.cuda.synchronize()
        spans = {name: [] for name, _, _ in PHASES}
        skew, net = [], []
        for _ in range(a.reps):
            evict.fill_(1)
            run_case(case, mode == 3)
            torch.cuda.synchronize()
            if lib.mi355_bn_resident_stamps(buf.ctypes.data) != 0:
                sys.exit('reading the stamps failed')
            s = buf[:n].astype(np.int64) * 0.01           # 100 MHz ticks -> us
            for name, i, j in PHASES:
                spans[name].extend(s[:, j] - s[:, i])
            skew.append(s[:, 2].max() - s[:, 2].min())
            net.extend(s[:, 3] - s[:, 2].max())
        cells = ['%6.2f /%6.2f' % (np.median(spans[name]), np.max(spans[name])) for name, _, _ in PHASES]
        print('%-22s %5d | %s | %6.2f /%6.2f | %6.2f /%6.2f' % ('rows%d C%d relu%d' % (rows, C, mode), n, ' | '.join(cells),
                                                              np.median(skew), np.max(skew), np.median(net), np.max(net)))
        del case
    if ops.bn_resident_timeouts():
        sys.exit('a block gave up: the figures above are void')


if __name__ == '__main__':
    main()
