"""Generate the mean-teacher golden vectors by calling the reference's live mt_loss (uda/model/loss.py:265-297; run where the
reference tree is present).  Writes tests/golden/g12_mt.npz.  Import recipe as make_golden_ema.py: namespace stubs for the
reference's packages; no reference source is copied, only arrays are stored.

    python tests/golden/make_golden_mt.py

Two cases, B = 2, K = 21: heat-maps of 8 x 8 (`a`) and 5 x 7 (`b`).  Stored per case: `<c>/pre`, `<c>/label`, `<c>/weight`, and for
every k in KS the fp32 loss `<c>/loss_<k>` and its gradient w.r.t. pre (torch autograd) on the channels that are not zero
throughout, `<c>/grad_<k>` (2, n, H, W), with their indices `<c>/joints_<k>` (n,): what mt_loss(k) selects is read off the
reference's own gradient, not restated here.  Where the gradient of k equals, bit for bit, that of an earlier k of the list, only
`<c>/grad_as_<k>` = that earlier k is stored.  About 75 KB of random fp32: the operands of these shapes alone are 33 KB."""
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

KS = (0, 99, 100, 199, 200, 299, 300, 399, 400, 1000)


def main():
    gen = torch.Generator().manual_seed(1208)
    out = {}
    for tag, (H, W) in (('a', (8, 8)), ('b', (5, 7))):
        pre = torch.randn(2, 21, H, W, generator=gen)
        label = torch.rand(2, 21, H, W, generator=gen)
        weight = torch.ones(2, 21, 1)
        out.update({tag + '/pre': pre.clone(), tag + '/label': label.clone(), tag + '/weight': weight})
        seen = []
        for k in KS:
            p = pre.clone().requires_grad_(True)
            loss = ref_loss.mt_loss(p, label, weight, k)
            loss.backward()
            out['%s/loss_%d' % (tag, k)] = loss.detach().clone()
            live = torch.nonzero(p.grad.abs().amax(dim=(0, 2, 3)) > 0).flatten()
            out['%s/joints_%d' % (tag, k)] = live.to(torch.int32)
            twin = [q for q, gq in seen if torch.equal(gq, p.grad)]
            if twin:
                out['%s/grad_as_%d' % (tag, k)] = torch.tensor(twin[0], dtype=torch.int32)
            else:
                out['%s/grad_%d' % (tag, k)] = p.grad[:, live].clone()
                seen.append((k, p.grad.clone()))
    arrs = {k: v.numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, 'g12_mt.npz'), **arrs)
    print('g12_mt', len(arrs), 'arrays')


if __name__ == '__main__':
    main()
