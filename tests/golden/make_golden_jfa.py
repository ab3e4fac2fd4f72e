"""Generate the joint-feature-alignment golden vectors by calling the reference's own loss1 and loss3 (uda/model/loss.py:331-378;
run where the reference tree is present).  Writes tests/golden/g15_jfa.npz.  Import recipe as make_golden_mmd.py: namespace stubs
for the reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_jfa.py

The reference hard-codes 21 joints and the upper clamp 63, so every case is 64 x 64 with K = 21 and coordinates in [0, 63].
Features are non-negative and dyadic (randint(0, 16) / 8: they compress well and are exact in bf16).  Cases:
  `a`  B = 2, C = 8: the designed key points below on both sides (in different joint orders)
  `b`  B = 1, C = 8: random integer and non-integer key points, the target features sparse (three quarters zero, as after a ReLU)
The designed key points (x, y): the four corners; (0, 63) and (63, 0), so that a swapped axis shows; 5 and 58 (a window cut on one
side) on either axis; three joints on one pixel; non-integer coordinates such as (10.7, 20.2); (0, 0) pairs as zeroed predictions.
Stored per case: `<c>/f1`, `<c>/f2` (B, C, 64, 64) fp32, `<c>/pre1`, `<c>/pre2` (B, 21, 2) fp32, the reference's `<c>/desc1`,
`<c>/desc2` = loss1 of either side, `<c>/loss`, `<c>/grad_f1`, `<c>/grad_f2` = loss3 and torch autograd in fp32, and the same from
the reference run on the float64 copies of the operands: `<c>/desc1_64`, `<c>/desc2_64`, `<c>/loss64`, `<c>/grad_f1_64`,
`<c>/grad_f2_64`.  About 0.3 MB."""
import os
import sys
import types
import numpy as np
import torch

REF = os.environ.get('REFERENCE_ROOT', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
np.int = int
np.float = float


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub('utils', f'{REF}/utils')
_stub('uda', f'{REF}/uda')
_stub('uda.model', f'{REF}/uda/model')
_stub('uda.model.resnet', _resnet=None, Bottleneck=None)

import uda.model.loss as ref_loss  # noqa: E402

DESIGNED = [(0, 0), (63, 63), (0, 63), (63, 0), (5, 30), (30, 5), (58, 30), (30, 58), (5, 58), (58, 5),
            (20, 33), (20, 33), (20, 33), (10.7, 20.2), (40.5, 12.9), (33.3, 47.8), (62.6, 6.1), (0, 0), (0, 0), (17, 41), (25, 28)]


def features(gen, B, C, sparse=False):
    f = torch.randint(0, 16, (B, C, 64, 64), generator=gen).float() / 8
    if sparse:
        f = f * (torch.rand(B, C, 64, 64, generator=gen) < 0.25).float()
    return f.contiguous()


def run(f1, f2, pre1, pre2, dtype):
    a = f1.to(dtype).clone().requires_grad_(True)
    b = f2.to(dtype).clone().requires_grad_(True)
    p1, p2 = pre1.to(dtype), pre2.to(dtype)
    loss = ref_loss.loss3(a, b, p1, p2)
    loss.backward()
    with torch.no_grad():
        d1, d2 = ref_loss.loss1(a, p1), ref_loss.loss1(b, p2)
    return d1.clone(), d2.clone(), loss.detach().clone(), a.grad.clone(), b.grad.clone()


def main():
    gen = torch.Generator().manual_seed(1510)
    d = torch.tensor(DESIGNED, dtype=torch.float32)
    assert d.shape == (21, 2)
    cases = {}
    pre1 = torch.stack([d, d.flip(0)])
    pre2 = torch.stack([d.roll(5, 0), d.flip(1)])
    cases['a'] = (features(gen, 2, 8), features(gen, 2, 8), pre1, pre2)
    rnd = torch.rand(1, 21, 2, generator=gen) * 63
    cases['b'] = (features(gen, 1, 8), features(gen, 1, 8, sparse=True), rnd.clone(),
                  torch.randint(0, 64, (1, 21, 2), generator=gen).float())
    out = {}
    for tag, (f1, f2, p1, p2) in cases.items():
        assert float(p1.min()) >= 0 and float(p1.max()) <= 63 and float(p2.min()) >= 0 and float(p2.max()) <= 63
        out[tag + '/f1'], out[tag + '/f2'], out[tag + '/pre1'], out[tag + '/pre2'] = f1.clone(), f2.clone(), p1.clone(), p2.clone()
        (out[tag + '/desc1'], out[tag + '/desc2'], out[tag + '/loss'], out[tag + '/grad_f1'], out[tag + '/grad_f2']) = run(f1, f2, p1, p2, torch.float32)
        (out[tag + '/desc1_64'], out[tag + '/desc2_64'], out[tag + '/loss64'], out[tag + '/grad_f1_64'],
         out[tag + '/grad_f2_64']) = run(f1, f2, p1, p2, torch.float64)
        assert out[tag + '/loss'].dtype == torch.float32 and out[tag + '/loss64'].dtype == torch.float64
    arrs = {k: v.numpy() for k, v in out.items()}
    path = os.path.join(HERE, 'g15_jfa.npz')
    np.savez_compressed(path, **arrs)
    print('g15_jfa', len(arrs), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
