"""Generate the MMD golden vectors by calling the reference's own MMD_loss3 and MMD_loss (uda/model/loss.py:1061-1196; run where
the reference tree is present).  Writes tests/golden/g14_mmd.npz.  Import recipe as make_golden_mt.py: namespace stubs for the
reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_mmd.py

Cases: `a` B = 2, K = 21, 8 x 8, randn source and a shifted, scaled randn target; `b` B = 3, K = 21, 5 x 7, the same kind; `c`
B = 4, K = 21, 8 x 8, Gaussian-blob heat-maps with noise (the regime the network produces); `d` MMD_loss on (5, 70) features.
Stored per case: `<c>/source`, `<c>/target` (fp32), the reference's fp32 result `<c>/loss`, `<c>/grad_source`, `<c>/grad_target`
(torch autograd) and the same from the reference run on the float64 copies of the operands, `<c>/loss64`, `<c>/grad_source64`,
`<c>/grad_target64`.  About 330 KB: 32 bytes of random numbers per operand element (fp32 operand and gradient, float64 gradient, on both
sides), 10 619 elements a side over the four cases."""
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


def blobs(gen, B, K, H, W, jitter):
    """Gaussian blobs (sigma 1) at random centres, peak near 1, plus noise of 0.02: what a trained head puts out."""
    cy = torch.rand(B, K, 1, 1, generator=gen) * (H - 1)
    cx = torch.rand(B, K, 1, 1, generator=gen) * (W - 1)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    g = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 2.0)
    return (g * (1.0 - jitter * torch.rand(B, K, 1, 1, generator=gen)) + 0.02 * torch.randn(B, K, H, W, generator=gen)).contiguous()


def run(crit, source, target, dtype):
    s = source.to(dtype).clone().requires_grad_(True)
    t = target.to(dtype).clone().requires_grad_(True)
    loss = crit(s, t)
    loss.backward()
    return loss.detach().clone(), s.grad.clone(), t.grad.clone()


def main():
    gen = torch.Generator().manual_seed(1410)
    cases = {}
    cases['a'] = (ref_loss.MMD_loss3(), torch.randn(2, 21, 8, 8, generator=gen), 0.7 * torch.randn(2, 21, 8, 8, generator=gen) + 0.3)
    cases['b'] = (ref_loss.MMD_loss3(), torch.randn(3, 21, 5, 7, generator=gen), 1.4 * torch.randn(3, 21, 5, 7, generator=gen) - 0.2)
    cases['c'] = (ref_loss.MMD_loss3(), blobs(gen, 4, 21, 8, 8, 0.1), blobs(gen, 4, 21, 8, 8, 0.5))
    cases['d'] = (ref_loss.MMD_loss(), torch.randn(5, 70, generator=gen), 0.8 * torch.randn(5, 70, generator=gen) + 0.5)
    out = {}
    for tag, (crit, source, target) in cases.items():
        out[tag + '/source'], out[tag + '/target'] = source.clone(), target.clone()
        out[tag + '/loss'], out[tag + '/grad_source'], out[tag + '/grad_target'] = run(crit, source, target, torch.float32)
        out[tag + '/loss64'], out[tag + '/grad_source64'], out[tag + '/grad_target64'] = run(crit, source, target, torch.float64)
        assert out[tag + '/loss'].dtype == torch.float32 and out[tag + '/loss64'].dtype == torch.float64
    arrs = {k: v.numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, 'g14_mmd.npz'), **arrs)
    print('g14_mmd', len(arrs), 'arrays')


if __name__ == '__main__':
    main()
