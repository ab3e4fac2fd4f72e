"""Generate the prototype-alignment golden vectors by calling the reference's own lossx and lossx3 (uda/model/loss.py:381-466,
560-652; run where the reference tree is present).  Writes tests/golden/g16_proto.npz.  Import recipe as make_golden_jfa.py:
namespace stubs for the reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_proto.py

The reference hard-codes 21 joints, the radius 6, the upper clamp 63 and m = 0.999, so every case is 64 x 64 with K = 21 and
coordinates in [0, 63].  Features are non-negative and dyadic (randint(0, 8) / 4: exact in bf16; stored as uint8 codes f * 4 under `f1_q4`, `f2_q4`).  Each
class runs as a sequence of three calls on ONE instance with fresh operands per call, so that the memories val1 / val2 of calls
two and three are the prototypes of the call before; both classes see the same operands, which are stored once.  Cases:
  `a`  B = 2, C = 8: the DESIGNED key points of make_golden_jfa.py on both sides, in joint orders that differ between the sides
       and from call to call
  `b`  B = 1, C = 8: random non-integer key points, the target features sparse (three quarters zero, as after a ReLU)
The source features (f2) are dense and strictly positive somewhere in every window: no source prototype sums to 0 (asserted).
Stored per case and call i = 0, 1, 2: `<c>/<i>/f1_q4`, `f2_q4` (B, C, 64, 64) uint8, `pre1`, `pre2` (B, 21, 2) fp32; per class
<k> = `x` (lossx) or `x3` (lossx3): `<c>/<i>/<k>/loss`, `grad_f1`, `grad_f2`, `val1`, `val2` from the fp32 run and the same with the
suffix `_64` from the run on the float64 copies of the operands.  About 0.4 MB."""
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
CALLS = 3
QUANT = 4          # features are multiples of 1 / QUANT in [0, 2): stored as their uint8 codes f * QUANT


def features(gen, B, C, sparse=False, low=0):
    f = torch.randint(low, 8, (B, C, 64, 64), generator=gen).float() / QUANT
    if sparse:
        f = f * (torch.rand(B, C, 64, 64, generator=gen) < 0.25).float()
    return f.contiguous()


def run(cls, calls, dtype):
    """Three consecutive calls on one instance: [(loss, grad_f1, grad_f2, val1, val2)] per call."""
    crit, out = cls(), []
    for f1, f2, pre1, pre2 in calls:
        a = f1.to(dtype).clone().requires_grad_(True)
        b = f2.to(dtype).clone().requires_grad_(True)
        loss = crit(a, b, pre1.to(dtype), pre2.to(dtype))
        loss.backward()
        assert crit.val1.dtype == dtype and not crit.val1.requires_grad and bool(torch.isfinite(loss))
        assert float(crit.val2.sum(-1).min()) > 0, 'a source prototype sums to 0'
        out.append((loss.detach().clone(), a.grad.clone(), b.grad.clone(), crit.val1.clone(), crit.val2.clone()))
    return out


def main():
    gen = torch.Generator().manual_seed(1610)
    d = torch.tensor(DESIGNED, dtype=torch.float32)
    assert d.shape == (21, 2)
    cases = {'a': [], 'b': []}
    for i in range(CALLS):
        pre1 = torch.stack([d.roll(i, 0), d.flip(0).roll(2 * i, 0)])
        pre2 = torch.stack([d.roll(5 + 3 * i, 0), d.flip(1).roll(i, 0)])
        cases['a'].append((features(gen, 2, 8), features(gen, 2, 8, low=1), pre1, pre2))
        cases['b'].append((features(gen, 1, 8, sparse=True), features(gen, 1, 8, low=1), torch.rand(1, 21, 2, generator=gen) * 63,
                           torch.rand(1, 21, 2, generator=gen) * 63))
    out = {}
    for tag, calls in cases.items():
        for i, (f1, f2, p1, p2) in enumerate(calls):
            assert float(p1.min()) >= 0 and float(p1.max()) <= 63 and float(p2.min()) >= 0 and float(p2.max()) <= 63
            for name, v in (('f1', f1), ('f2', f2)):
                code = (v * QUANT).to(torch.uint8)
                assert torch.equal(code.float() / QUANT, v)
                out['%s/%d/%s_q%d' % (tag, i, name, QUANT)] = code
            out['%s/%d/pre1' % (tag, i)], out['%s/%d/pre2' % (tag, i)] = p1.clone(), p2.clone()
        for k, cls in (('x', ref_loss.lossx), ('x3', ref_loss.lossx3)):
            for dtype, suffix in ((torch.float32, ''), (torch.float64, '_64')):
                for i, res in enumerate(run(cls, calls, dtype)):
                    for name, v in zip(('loss', 'grad_f1', 'grad_f2', 'val1', 'val2'), res):
                        assert v.dtype == dtype and bool(torch.isfinite(v).all())
                        out['%s/%d/%s/%s%s' % (tag, i, k, name, suffix)] = v
    arrs = {k: v.numpy() for k, v in out.items()}
    path = os.path.join(HERE, 'g16_proto.npz')
    np.savez_compressed(path, **arrs)
    print('g16_proto', len(arrs), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
